"""The margin families of tests/wide_margin_scenes.py on the CPU: the model puts them where it says it does (a changed generator cannot silently leave
the boundary of the fold's trust test), the oracle answers all of them sensibly and with the tie rule the GPU must reproduce, and -- in the build container --
the oracle equals the reference's own compiled renderer on one frame per family, so that "GPU == oracle" (tests/test_gpu_wide_margins.py) means "GPU ==
reference" on geometry this odd too."""
import os
import tempfile

import numpy as np
import pytest

import oracle_lib
import ray_query_shim as shim
import raytracer_amd as ra
import ref_render
import wide_margin_scenes as wm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def trusted_share(scene, rays):
    base, step, bound, holds = wm.scene_grid(scene)
    trusted, untrusted, borderline = wm.trust_model(rays, base, step, bound)
    assert not (trusted & untrusted).any() and (trusted | untrusted | borderline).all()
    return holds, float(trusted.mean()), float(untrusted.mean())


@pytest.mark.parametrize("axis", sorted(wm.OFFSETS))
def test_model_shares_of_the_offset_family(built, axis):
    """aimed(1.5) rays: one displacement with >= 0.95 clearly trusted, at least two with the share in 0.1 .. 0.9, one with none, one without a grid."""
    ks = wm.OFFSETS[axis]
    shares = {}
    for k in (ks["trusted"],) + tuple(ks["borderline"]) + (ks["untrusted"], ks["no_grid"]):
        pos, idx = wm.offset_mesh(k, axis)
        scene = wm.single_mesh_scene(pos, idx)
        shares[k] = trusted_share(scene, wm.aimed(scene, pos, 1.5))
        print(axis, k, shares[k])
    assert shares[ks["trusted"]][0] and shares[ks["trusted"]][1] >= 0.95
    assert len(ks["borderline"]) >= 2
    for k in ks["borderline"]:
        assert shares[k][0] and 0.1 < shares[k][1] < 0.9, (k, shares[k])
    assert shares[ks["untrusted"]][0] and shares[ks["untrusted"]][1] == 0.0 and shares[ks["untrusted"]][2] == 1.0
    assert not shares[ks["no_grid"]][0]


def test_model_shares_of_the_aimed_family(built):
    """On the centred sheet the start distances run from all rays trusted to none."""
    pos, idx = wm.offset_mesh(0.0, "x")
    scene = wm.single_mesh_scene(pos, idx)
    shares = [trusted_share(scene, wm.aimed(scene, pos, d)) for d in wm.AIMED_DISTANCES]
    print(list(zip(wm.AIMED_DISTANCES, shares)))
    assert all(s[0] for s in shares)
    t = [s[1] for s in shares]
    assert wm.AIMED_DISTANCES == (1.5, 10.0, 30.0, 80.0, 1e3, 1e5)
    assert t[0] >= 0.95 and t[1] >= 0.9 and 0.1 < t[2] < 0.9 and 0.0 < t[3] < 0.1 and t[4] == 0.0 and t[5] == 0.0
    assert all(a >= b for a, b in zip(t, t[1:]))
    assert shares[4][2] == 1.0 and shares[5][2] == 1.0


def test_model_classes_of_tiny_components_and_flat_meshes(built):
    """A direction component of 1e-39 or 1e-44 (float32 denormals) has an infinite quotient without being zero, one of 1e-37 a finite one: the first two are
    clearly untrusted whatever the mesh, the others follow the mesh.  A flat mesh at y = 0 has a grid whose step on the flat axis is 1e-6 of the largest over
    65527: no aimed ray is trusted but one that starts in the plane; the same sheet at y = 0.25 has no grid."""
    pos, idx = wm.offset_mesh(0.0, "x")
    scene = wm.single_mesh_scene(pos, idx)
    rays = wm.tiny_components(scene, pos)
    base, step, bound, holds = wm.scene_grid(scene)
    trusted, untrusted, _ = wm.trust_model(rays, base, step, bound)
    i = np.arange(len(rays))
    value = np.asarray(wm.TINY)[(i // 3) % len(wm.TINY)]
    assert np.array_equal(rays[i, 4 + i % 3], value.astype(np.float32)) and np.all(rays[i, 4 + i % 3] != 0.0)
    d = rays[:, 4:7].astype(np.float64)
    quotient = np.linalg.norm(d, axis=1) / np.abs(d[i, i % 3])   # of the normalised component (a short direction brings 1e-39 back into range)
    assert untrusted[quotient > 1.02 * wm.FLT_MAX].all() and not untrusted[quotient < 0.5 * wm.FLT_MAX].any()
    assert untrusted[np.abs(value) < 1e-38].mean() > 0.9
    assert trusted[np.abs(value) > 1e-38].mean() > 0.95
    for y, expected in ((0.0, True), (0.25, False)):
        fpos, fidx = wm.flat_mesh(y)
        flat = wm.single_mesh_scene(fpos, fidx)
        holds, share, _ = trusted_share(flat, wm.aimed(flat, fpos, 1.5))
        assert holds == expected and share < 1e-3   # (a ray that starts within 3e-5 of the plane)


FAMILIES = wm.mesh_families()


@pytest.mark.parametrize("name", list(FAMILIES))
def test_oracle_answers_every_family(built, name):
    """Hit share between 0.05 and 0.95 for closest-hit and any-hit queries on every mesh family and every ray family it meets on the device.
    The tie rule, on layers with exactly duplicated sheets: of equal distances the first one found in the reference's order stands (`distance < best`), and that
    order is the ray's own -- the eight coincident triangles lie in different leaves, visited nearest box first by the ray's direction signs.  So the reported
    triangles come from several sheets across the rays, while distance and barycentrics are those of a single sheet bit for bit.  The GPU comparison holds the triangle index word for word, i.e. the same winner per ray."""
    pos, idx = FAMILIES[name]
    scene = wm.single_mesh_scene(pos, idx)
    for family in wm.families_of(name):
        rays = wm.ray_families(scene, pos, idx, family)
        assert rays.shape == (wm.NUM_RAYS, 8) and np.isfinite(rays[:, 0:3]).all() and np.isfinite(rays[:, 4:7]).all()
        hits, _, _ = shim.closest(scene.desc, rays, surfaces=False)
        occ, _ = shim.any_hit(scene.desc, rays)
        share = float((hits[:, 1] != ra.RT_INVALID_OBJECT).mean())
        print(name, family, share, float(occ.mean()))
        assert 0.05 < share < 0.95, (name, family, share)
        assert 0.05 < occ.mean() < 0.95, (name, family)
        if name in ("layers_y_0", "layers_oblique_0"):
            sheets = np.unique(wm.hit_sheet(scene, hits))
            assert len(sheets[sheets >= 0]) >= 2, (name, family, sheets.tolist())
            if family == "aimed_1.5":
                # (not the grazing rays: through a vertex or along an edge a hit also depends on the leaf boxes around it -- the reference's walk tests them
                # first -- and those are another tree's in the single sheet)
                one_pos, one_idx = pos[:len(pos) // wm.LAYER_SHEETS], idx[:len(idx) // wm.LAYER_SHEETS]
                one_scene = wm.single_mesh_scene(one_pos, one_idx)
                one, _, _ = shim.closest(one_scene.desc, rays, surfaces=False)
                assert np.array_equal(one[:, [0, 1, 3, 4]], hits[:, [0, 1, 3, 4]])   # distance, object, u, v


def test_the_layer_sweep_places_runner_ups_inside_the_tolerance(built):
    """wide_margin_scenes.must_retrace over the oblique layers: in total at least 1 000 rays whose runner-up lies between tol / 4 and tol of their best hit (the
    rays that tell RT_WIDE_FOLD_TOL from a tolerance four times narrower), and with exact duplicates every robust ray has its runner-up AT its best."""
    total = 0
    for k in wm.LAYER_ULPS:
        pos, idx = wm.layers_mesh(k, True)
        scene = wm.single_mesh_scene(pos, idx)
        must, band = wm.must_retrace(scene, pos, idx, wm.aimed(scene, pos, 1.5), True)
        print(k, int(must.sum()), int(band.sum()))
        assert not (band & ~must).any() and (k != 0 or (must.sum() > 1000 and band.sum() == 0))
        total += int(band.sum())
    assert total >= 1000


def test_two_level_scenes_are_answered_too(built):
    pos, idx = wm.offset_mesh(wm.OFFSETS["diag"]["borderline"][1], "diag")
    scene = wm.two_level_scene(pos, idx)
    d = scene.desc.contents
    assert d.numObjects == 3 and d.numMeshes == 1 and d.numTopNodes > 0   # the second mesh object is an instance: one mesh, one tree
    rays = wm.two_level_rays(scene, pos)
    hits, _, _ = shim.closest(scene.desc, rays, surfaces=False)
    hit = hits[:, 1] != ra.RT_INVALID_OBJECT
    assert 0.05 < hit.mean() < 0.95
    assert set(np.unique(hits[hit, 1]).tolist()) == {0, 1, 2} and len(wm.mesh_objects(scene)) == 2   # both mesh objects and the sphere


# one frame per family through the reference's own renderer
REFERENCE_FRAMES = ("offset_borderline", "offset_no_grid", "layers_oblique_1", "rect_below_1", "point_homothetic", "flat_0", "sliver_box")


def _family_frame(name, aspect):
    if name in wm.FRAME_CASES:
        return wm.frame_case(name, aspect)[:2]
    pos, idx = wm.flat_mesh(0.0) if name == "flat_0" else wm.sliver_box_mesh()
    size = pos.max(0).astype(np.float64) - pos.min(0)
    centre = 0.5 * (pos.max(0).astype(np.float64) + pos.min(0))
    reach = float(size[2])   # the sliver box: the camera looks at one end-to-end unit of it
    return wm.single_mesh_scene(pos, idx, wm._sheet_lights(centre, (0.0, 1.0, 0.0), reach)), wm._sheet_camera(centre, (0.0, 1.0, 0.0), reach, aspect)


@pytest.mark.parametrize("name", REFERENCE_FRAMES)
def test_oracle_equals_the_reference_renderer_on_the_margin_families(built, name):
    """The path tools/reference_fuzz.py takes: tests/ref_render.py's export_scene and run, the oracle in its x86 approximation mode, 1 pass, depth 3, 48 x 32,
    every pixel and the ray counters bit for bit.  Build container only, skipped elsewhere exactly as tests/test_reference_soak.py is.
    Not exported: the two_level family -- its second object is a Scene.add_instance, which the scene file of oracle/ref_harness/ref_render.cpp has no record
    for (the exporter raises on it); its meshes are covered here as single objects and its top level by the soak's random two-level scenes."""
    if not os.path.exists(os.path.join(ROOT, "oracle", "_ref", "ref_render")):
        pytest.skip("oracle/_ref/ref_render is built from /root/reference (build container only)")
    ok, _ = oracle_lib.set_x86_approximations(True)
    if not ok:
        oracle_lib.set_x86_approximations(False)
        pytest.skip("this CPU cannot evaluate the reference's approximate instructions")
    try:
        w, h, depth, dims, seed = 48, 32, 3, 128, 4321
        scene, camera = _family_frame(name, w / h)
        desc = scene.desc
        assert 3 * desc.contents.numLights + 4 <= (dims - 4) // (depth + 1)   # paths stay inside the sampler's dimensions (tools/reference_fuzz.py says why)
        with tempfile.TemporaryDirectory(prefix="rt_margins_", dir="/tmp") as tmp:
            path = os.path.join(tmp, "scene.bin")
            ref_render.export_scene(path, scene, camera, w, h, 1, 1, depth, dimensions=dims, light_sampling_all=True, seed=seed)
            _, out = ref_render.run(path, threads=1)
        bn = ra.load_blue_noise()
        desc.contents.blueNoise = bn.ctypes.data
        vp = ra.Viewport(w, h, seed=seed, max_ray_depth=depth, light_sampling_all=True, dimensions=dims)
        vp.reset()
        img, cnt = np.zeros((h, w, 3), dtype=np.float32), np.zeros(16, dtype=np.uint64)
        p = vp.next_pass_params(camera)
        oracle_lib.render_pass(desc, p, w, h, img, None, cnt, threads=4)
        assert np.array_equal(np.ctypeslib.as_array(p.seed, shape=(p.numDimensions,)), out["first_pass_seeds"])
        differing = int(np.count_nonzero((img.view(np.uint32) != out["image"].view(np.uint32)).any(axis=2)))
        print(name, "rays", int(cnt[0]), out["numRays"], "shadow", int(cnt[1]), out["numShadowRays"], int(cnt[2]), out["numShadowRaysHit"], "pixels differing", differing)
        assert int(cnt[8]) > 0 and int(cnt[1]) > 0   # the frame sees the mesh and samples its lights
        assert (int(cnt[0]), int(cnt[1]), int(cnt[2])) == (out["numRays"], out["numShadowRays"], out["numShadowRaysHit"])
        assert differing == 0
    finally:
        oracle_lib.set_x86_approximations(False)
