"""The 4-wide walks held to the oracle where their exactness margins are thin (rt_wide_grid.inl, rt_wide_walk.h): geometry displaced from its own origin
until the fold's trust test turns, rays that start ever farther away, direction components with huge or infinite quotients, rays through vertices, edges,
hit points and leaf-box corners, stacks of sheets 0 .. 65536 ulps apart (the runner-up tolerance), flat and sliver-shaped boxes (the grid's step), and
lights flush with geometry (the any-hit leaf gate against the fixed ray length).  Families and the model of the margins: tests/wide_margin_scenes.py;
their CPU side: tests/test_wide_margins_cpu.py.

Every comparison is word for word.  Each test also shows that it is about what it claims: the walk that served it (rtgpu_get_update_info) is the one the
model predicts, and the walk's own tallies -- rays it did not trust, rays it handed to the binary walk -- lie where the model puts them."""
import ctypes as C

import numpy as np
import pytest

import ray_query_shim as shim
import raytracer_amd as ra
import wide_margin_scenes as wm
from test_gpu_parity import assert_identical, run_both
from test_gpu_ray_queries import viewport

pytestmark = pytest.mark.gpu

FAMILIES = wm.mesh_families()
BENIGN_MESHES = ("centred",) + tuple("offset_%s_%g" % (axis, wm.OFFSETS[axis]["trusted"]) for axis in sorted(wm.OFFSETS))
QUERY_CASES = [(m, f) for m in FAMILIES for f in wm.families_of(m)]
# the centred sheet under the start distances: the clearly trusted share the model gives (tests/test_wide_margins_cpu.py asserts the same figures)
CENTRED_SHARES = {"aimed_1.5": (0.95, 1.0), "aimed_10": (0.9, 1.0), "aimed_30": (0.1, 0.9), "aimed_80": (0.0, 0.1), "aimed_1000": (0.0, 0.0), "aimed_100000": (0.0, 0.0)}

_contexts, _references = {}, {}


def _context(mesh, walk):
    """scene and viewport of a mesh family member: kept for the cases that follow it (two meshes' worth: both walks of one mesh)"""
    key = (mesh, walk)
    if key not in _contexts:
        while len(_contexts) >= 2:
            _contexts.pop(next(iter(_contexts)))
        pos, idx = FAMILIES[mesh]
        scene = wm.single_mesh_scene(pos, idx)
        _contexts[key] = (scene, viewport(scene, walk))
    return _contexts[key]


def _reference(mesh, family, scene):
    """rays and the oracle's answers, computed once for both walks and left unchanged"""
    key = (mesh, family)
    if key not in _references:
        while len(_references) >= 2:
            _references.pop(next(iter(_references)))
        pos, idx = FAMILIES[mesh]
        rays = wm.ray_families(scene, pos, idx, family)
        hits, surf, _ = shim.closest(scene.desc, rays)
        occ, _ = shim.any_hit(scene.desc, rays)
        for a in (rays, hits, surf, occ):
            a.setflags(write=False)
        _references[key] = (rays, hits, surf, occ)
    return _references[key]


def trace(vp, mode, rays, surfaces=True):
    """rtgpu_trace_rays on raw records: (hits, surfaces, occluded, the query arena's RtCounters -- _reserved[0]: rays k_trace_wide did not trust)"""
    lib = ra.rtgpu_lib()
    n = len(rays)
    hits = np.zeros((n, 8), dtype=np.uint32) if mode == ra.TRACE_CLOSEST else None
    surf = np.zeros((n, 12), dtype=np.uint32) if (surfaces and mode == ra.TRACE_CLOSEST) else None
    occ = np.zeros(n, dtype=np.uint32) if mode == ra.TRACE_ANY else None
    stats = ra.RtCounters()
    p = lambda a: a.ctypes.data_as(C.c_void_p) if a is not None else None   # noqa: E731
    r = lib.rtgpu_trace_rays(vp.device_context(), C.c_uint32(mode), p(np.ascontiguousarray(rays)), C.c_uint32(n), p(hits), p(surf), p(occ), C.byref(stats))
    assert r == 0, lib.rtgpu_last_error()
    return hits, surf, occ, stats


def check_grid(vp, scene, serving):
    """the model's grid is the device's: (base, step, bound, holds) with base / step / bound read back from the level that serves object 0"""
    base, step, bound, holds = wm.scene_grid(scene)
    if serving == "wide":
        info, _, _ = ra.read_wide_level(vp.device_context(), 0)
        for mine, name in ((base, "base"), (step, "step"), (bound, "bound")):
            assert np.array_equal(mine.view(np.uint32), info[name].view(np.uint32)), (name, mine, info[name])
    return base, step, bound, holds


def describe(bad, rays, trusted, untrusted, got, expected):
    return ("%d rays differ; first: " % len(bad)) + "; ".join("ray %d (%s) %s gpu %s oracle %s" % (i, wm.model_class(trusted, untrusted, i), rays[i].tolist(), got[i].tolist(), expected[i].tolist())
                                                             for i in bad[:3])


@pytest.mark.parametrize("case", QUERY_CASES, ids=["%s-%s" % c for c in QUERY_CASES])
def test_queries_on_the_margins_equal_the_oracle(built, walk, case):
    mesh, family = case
    scene, vp = _context(mesh, walk)
    rays, ref_hits, ref_surf, ref_occ = _reference(mesh, family, scene)
    n = len(rays)
    serving = ra.update_info(vp.device_context())["walk"]
    base, step, bound, holds = check_grid(vp, scene, serving)
    assert serving == (("wide" if holds else "binary") if walk == "default" else "binary"), (mesh, serving, holds)
    trusted, untrusted, _ = wm.trust_model(rays, base, step, bound)
    hits, surf, _, stats = trace(vp, ra.TRACE_CLOSEST, rays)
    print("%s %s %s: walk %s, model trusted %d untrusted %d of %d; device untrusted %d retraced %d" %
          (mesh, family, walk, serving, trusted.sum(), untrusted.sum(), n, stats._reserved[0], stats.numRetracedRays))
    bad = np.nonzero((hits != ref_hits).any(axis=1))[0]
    assert len(bad) == 0, (mesh, family, walk, describe(bad, rays, trusted, untrusted, hits, ref_hits))
    bad = np.nonzero((surf != ref_surf).any(axis=1))[0]
    assert len(bad) == 0, (mesh, family, walk, describe(bad, rays, trusted, untrusted, surf, ref_surf))
    _, _, occ, _ = trace(vp, ra.TRACE_ANY, rays)   # (the binary walk under either setting: include/rtgpu.h)
    bad = np.nonzero(occ != ref_occ)[0]
    assert len(bad) == 0, (mesh, family, walk, describe(bad, rays, trusted, untrusted, occ[:, None], ref_occ[:, None]))
    if serving != "wide":
        assert stats.numRetracedRays == 0 and stats._reserved[0] == 0
        return
    # k_trace_wide tallies the rays its fold does not trust (rt_trace_wide.inl: numUntrusted -> RT_COUNTER_RETRACED + 1 = _reserved[0]); each of them is a
    # hand-over too
    assert untrusted.sum() <= stats._reserved[0] <= n - trusted.sum(), (mesh, family, int(untrusted.sum()), int(stats._reserved[0]), int(n - trusted.sum()))
    assert stats._reserved[0] <= stats.numRetracedRays <= n
    if mesh == "centred" and family in CENTRED_SHARES:
        lo, hi = CENTRED_SHARES[family]
        assert lo <= trusted.mean() <= hi, (family, float(trusted.mean()))
    if mesh in BENIGN_MESHES and family == "aimed_1.5":
        # a floor, not a performance bar: the 4-wide walk decided rays itself (the suite's benign scenes retrace under 2 %)
        assert trusted.sum() >= 0.95 * n and stats.numRetracedRays <= n - trusted.sum() / 2


@pytest.mark.parametrize("oblique", [False, True], ids=["y", "oblique"])
def test_retraces_fall_as_the_layers_part(built, oblique):
    """The runner-up sweep: eight sheets 0 .. 65536 ulps apart under aimed(1.5) rays.  With exact duplicates every ray that hits has a runner-up AT its best
    and is retraced; from "inside tol" to "clearly outside" the count may only fall (within a factor of two per step).  The stack with the normal along y is
    flat: up to 256 ulps it has no grid and the binary walk serves it (nothing to retrace), beyond it the sweep starts there.
    And per ray (wide_margin_scenes.must_retrace, oblique stack): the oracle on every sheet alone gives a ray's candidates, the model its tolerance; the rays
    whose runner-up lies clearly within tol of their best hit are sent as a batch of their own and ALL of them must come back retraced -- about 1 900 of them
    over the sweep have the runner-up beyond tol / 4, which a tolerance four times too narrow would decide itself."""
    counts, in_band = [], 0
    for k in wm.LAYER_ULPS:
        mesh = "layers_%s_%d" % ("oblique" if oblique else "y", k)
        pos, idx = FAMILIES[mesh]
        scene = wm.single_mesh_scene(pos, idx)
        vp = viewport(scene)
        serving = ra.update_info(vp.device_context())["walk"]
        holds = wm.scene_grid(scene)[3]
        assert serving == ("wide" if holds else "binary")
        rays = wm.aimed(scene, pos, 1.5)
        hits, _, _, stats = trace(vp, ra.TRACE_CLOSEST, rays, surfaces=False)
        ref_hits, _, _ = shim.closest(scene.desc, rays, surfaces=False)
        assert np.array_equal(hits, ref_hits)
        unbounded = rays.copy()
        unbounded[:, 3] = np.inf   # closest-hit rays are walked from +inf (include/rtgpu.h)
        found, _, _ = shim.closest(scene.desc, unbounded, surfaces=False)
        num_hit = int((found[:, 1] != ra.RT_INVALID_OBJECT).sum())
        print("layers k_ulps %d %s: walk %s, rays that hit %d, untrusted %d, retraced %d" % (k, "oblique" if oblique else "y", serving, num_hit, stats._reserved[0], stats.numRetracedRays))
        if serving == "wide":
            counts.append((k, int(stats.numRetracedRays), num_hit, int(stats._reserved[0])))
        else:
            assert not oblique and not counts and stats.numRetracedRays == 0
        if oblique:
            # per ray: those whose runner-up the model puts clearly within tol of their best hit, sent alone -- every one of them is handed over
            must, band = wm.must_retrace(scene, pos, idx, rays, True)
            in_band += int(band.sum())
            if must.any():
                sub_hits, _, _, sub_stats = trace(vp, ra.TRACE_CLOSEST, rays[must], surfaces=False)
                print("   runner-up within tol: %d rays (%d of them beyond tol / 4), retraced %d" % (must.sum(), band.sum(), sub_stats.numRetracedRays))
                assert np.array_equal(sub_hits, ref_hits[must])
                assert sub_stats.numRetracedRays == must.sum(), (k, int(must.sum()), int(band.sum()), int(sub_stats.numRetracedRays))
    assert len(counts) >= 2 and (not oblique or len(counts) == len(wm.LAYER_ULPS))
    if oblique:
        assert in_band >= 1000   # the sweep does place runner-ups between tol / 4 and tol
        k, retraced, num_hit, num_untrusted = counts[0]
        assert k == 0 and num_untrusted == 0 and retraced >= num_hit > 0.5 * len(rays)
        assert counts[-1][1] < 0.1 * counts[0][1]   # clearly outside: the sweep does reach the far end
    for (k0, r0, _, _), (k1, r1, _, _) in zip(counts, counts[1:]):
        assert r1 <= 2 * r0, (k0, r0, k1, r1)


@pytest.mark.parametrize("mesh", ["offset_diag_%g" % wm.OFFSETS["diag"]["borderline"][1], "layers_oblique_1"])
def test_two_level_queries_equal_the_oracle(built, walk, mesh):
    """The same meshes as two objects (the second an instance 1e3 extents away) and a far sphere: k_trace_wide2, whose mesh levels see local rays that came
    through invTransform at large magnitude.  (k_trace_wide2 keeps no untrusted tally -- rt_trace_wide2.inl -- and a ray reaches a mesh level only through
    the top level, so the model's per-ray classes bound nothing here: the walk and the answers are asserted.)"""
    pos, idx = FAMILIES[mesh]
    scene = wm.two_level_scene(pos, idx)
    rays = wm.two_level_rays(scene, pos)
    vp = viewport(scene, walk)
    assert ra.update_info(vp.device_context())["walk"] == ("wide2" if walk == "default" else "binary")
    ref_hits, ref_surf, _ = shim.closest(scene.desc, rays)
    hit = ref_hits[:, 1] != ra.RT_INVALID_OBJECT
    assert set(np.unique(ref_hits[hit, 1]).tolist()) == {0, 1, 2}
    hits, surf, _, stats = trace(vp, ra.TRACE_CLOSEST, rays)
    print("two_level %s %s: retraced %d of %d" % (mesh, walk, stats.numRetracedRays, len(rays)))
    bad = np.nonzero((hits != ref_hits).any(axis=1))[0]
    assert len(bad) == 0, (mesh, walk, len(bad), bad[:8].tolist(), rays[bad[:2]].tolist(), hits[bad[:2]].tolist(), ref_hits[bad[:2]].tolist())
    assert np.array_equal(surf, ref_surf)
    _, _, occ, _ = trace(vp, ra.TRACE_ANY, rays)
    ref_occ, _ = shim.any_hit(scene.desc, rays)
    assert np.array_equal(occ, ref_occ)


@pytest.mark.parametrize("name", wm.FRAME_CASES)
def test_frames_on_the_margins_equal_the_oracle(built, walk, name):
    """Frames, for the 4-wide ANY-HIT walk, which queries never reach: 64 x 40, 2 passes, depth 4, every light sampled at every vertex.
    numShadowRaysHit counts the next-event rays that REACH their light (PathTracerMIS::SampleLight).  Light gets through in every case but
    wide_margin_scenes.ALL_OCCLUDED (which says why, and why a light up to 64 ulps beyond a sheet is not shut off by it): there numShadowRaysHit is 0 of a
    positive numShadowRays -- asserted, so that two black frames cannot pass as agreement.
    The layers are staggered (every copy shows a strip beside the copies above it) under a point light 2 milliradians above their plane: a next-event ray leaves
    its strip 1e-4 along that direction, i.e. 2e-7 above its own sheet, and passes under copies k, 2 k, ... ulps higher -- the offset lands beyond them (k <= 1),
    on or between them (16, 256) or under all of them (4096); the oracle has 7, 11, 55, 131 and 1079 of ~5160 next-event rays occluded for k = 0, 1, 16, 256, 4096."""
    w, h = 64, 40
    scene, camera, serving = wm.frame_case(name, w / h)
    if walk == "default":
        assert ra.update_info(viewport(scene).device_context())["walk"] == serving
    out = run_both(scene, camera, w, h, walk=walk, passes=2, max_ray_depth=4, light_sampling_all=True)
    c = out[2]
    print("%s %s: walk %s, shadow rays %d, reached the light %d, mesh hits %d, analytic hits %d, retraced %d, untrusted %d" %
          (name, walk, serving, c["numShadowRays"], c["numShadowRaysHit"], c["numMeshHits"], c["numAnalyticHits"], c.get("numRetracedRays", 0), c.get("numUntrustedRays", 0)))
    assert_identical(*out)
    assert c["numMeshHits"] > 0
    if name in wm.ALL_OCCLUDED:
        assert c["numShadowRays"] > 0 and c["numShadowRaysHit"] == 0
    else:
        assert c["numShadowRays"] > c["numShadowRaysHit"] > 0
    if name.startswith("two_level"):
        assert c["numAnalyticHits"] > 0
