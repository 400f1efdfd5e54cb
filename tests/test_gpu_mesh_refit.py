"""rtgpu_update_mesh on the device (through Scene.set_mesh_vertices / Scene.update() / Viewport.update_scene() of the host mirror): a mesh whose vertices moved
is refitted in place from its new positions, and everything after it is held to the bar of every other scene.

  tables    rtgpu_read_mesh equals the NumPy model of the refit rules (tests/mesh_refit_ref.py) and rtgpu_read_wide_level equals the pure host function's
            tables -- computed on the CPU by tests/cpp/mesh_refit_check.cpp's emit mode, never by the device -- bit for bit, BEFORE anything is rendered on
            them.  The 4 096-triangle soup is the smallest mesh here with depths wider than the single-block kernel's 1 024 nodes: its depths 11 and 12
            (1 554 and 1 134 nodes) get a launch each, depths 13 .. 14 below them and 10 .. 0 above them run in one single-block launch each.
  render    sum buffer, secondary buffer and counters bit-identical to the CPU oracle on scene.desc after each update, under both walks (tests/conftest.py).
  96 x 64, 2 passes, depth 4."""
import ctypes as C

import numpy as np
import pytest

import oracle_lib
import raytracer_amd as ra
import mesh_refit_ref as ref
import mesh_refit_scenes as ms
import ray_query_shim as shim
import temporal_moving_ref as mref
import temporal_ref
import update_scenes as us
from test_gpu_parity import COMPARED, NOT_INTERSECTION, assert_identical
from test_gpu_ray_queries import device as query_device
from test_gpu_update import BLUE_NOISE, H, W, Oracle, assert_same_frames, frame, passes, viewport
from test_mesh_refit_cpu import bits, expected_tables, flattened

pytestmark = pytest.mark.gpu

OK, INVALID_ARGUMENT, NOT_READY, UNSUPPORTED = 0, -1, -5, -6
ASPECT = W / H
RENDER_MESH = "grid17"


@pytest.fixture(scope="module")
def expected(built, tmp_path_factory):
    """the pure host function's tables for every mesh at steps 0 (as uploaded), 1 and 2: computed once, on the CPU"""
    return expected_tables(tmp_path_factory.mktemp("refit"), (0, 1, 2))


def deform(scene, vp, pos, idx, step, with_normals):
    new = ms.deformed(pos, step)
    normals = ms.vertex_normals(new, idx) if with_normals else None
    scene.set_mesh_vertices(ms.MESH_OBJECT, new, normals, ms.vertex_tangents(normals) if with_normals else None)
    scene.update()
    vp.update_scene()
    return new


def mesh_objects(scene):
    """the flat objects that are the deforming mesh (leaf order)"""
    o, mi = scene.desc.contents, ms.mesh_index(scene)
    return [i for i in range(o.numObjects) if o.objects[i].objectKind == 0 and o.objects[i].shapeKind == 3 and o.objects[i].meshIndex == mi]


# ---- tables ------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", list(ms.SCENES))
@pytest.mark.parametrize("name", ms.MESHES)
def test_the_device_tables_equal_the_model_before_anything_is_rendered(built, expected, kind, name):
    scene, camera, pos, idx, nrm = ms.SCENES[kind](name, ASPECT)
    nodes0, indices, tris0 = ms.mesh_tables(scene)
    if name == "soup4096":
        widths = ref.depth_widths(nodes0)
        assert [d for d, n in enumerate(widths) if n > 1024] == [11, 12] and len(widths) == 15, widths     # which depths take which path (module docstring)
    vp = viewport(scene, "default")
    vp.update_scene()            # never uploaded: goes up whole
    ctx, mi = vp.device_context(), ms.mesh_index(scene)
    wide = not (kind == "single" and name in ("tri1", "tri2"))     # a single mesh whose root is a leaf has no 4-wide tree: the binary walk serves it

    def check(step, want_nodes, want_tris):
        nodes, tris = ra.read_mesh(ctx, mi, len(nodes0), len(indices))
        assert np.array_equal(nodes, want_nodes), (step, int(np.count_nonzero(nodes != want_nodes)))
        assert np.array_equal(bits(tris), bits(want_tris)), step
        if not wide:
            info = ra.RtWideLevelInfo()
            assert ra.rtgpu_lib().rtgpu_read_wide_level(ctx, 0, C.byref(info), None, C.c_uint64(0), None, C.c_uint64(0)) == NOT_READY
            return
        e = expected[(name, step)]
        for o in mesh_objects(scene):         # the instance's level record too
            info, records, gates = ra.read_wide_level(ctx, o)
            assert info["valid"] == 1
            if kind == "two_level" and name in ("tri3", "grid17", "soup4096"):
                # the prop's mesh lies in front of this one in every table: node, triangle, 4-wide node and gate ranges that do not start at 0
                assert mi == 1 and info["nodeBase"] > 0 and info["gateBase"] > 0 and info["triBase"] > 0
            for key in ("base", "step", "bound"):
                assert np.array_equal(bits(info[key]), bits(e[key])), (step, o, key, info[key], e[key])
            assert np.array_equal(records, e["records"]), (step, o, int(np.count_nonzero(records != e["records"])))
            assert np.array_equal(bits(gates), bits(e["gates"])), (step, o)

    check(0, nodes0, tris0)      # as uploaded: the tables a same-positions refit gives
    before = ra.update_info(ctx)
    assert before["numMeshUpdates"] == 0
    for step, with_normals in ((1, False), (2, True)):
        new = deform(scene, vp, pos, idx, step, with_normals)
        want_nodes, want_tris, _ = ref.refit(nodes0, indices, new)
        check(step, want_nodes, want_tris)
        info = ra.update_info(ctx)
        assert info["numMeshUpdates"] == step and info["walk"] == before["walk"]
        if kind == "single":     # (two-level: the objects update that follows is the last one, and bytesUploaded is the last update's)
            # positions, with normals the vertex shading too; the first update also brings the vertex indices (16 bytes a triangle) and the depth offsets
            assert 12 * len(pos) <= info["bytesUploaded"] <= (12 + 32 * with_normals) * len(pos) + (step == 1) * (16 * len(indices) + 4 * 66) + 32
            assert info["numUpdates"] == 0
    # the same positions again: the device's tables are a function of the positions alone
    scene.set_mesh_vertices(ms.MESH_OBJECT, pos)
    scene.update()
    vp.update_scene()
    check(0, nodes0, tris0)
    # ... and only now a frame on them, against the oracle
    oracle = Oracle()
    passes(vp, camera, 2, oracle, scene)
    got = frame(vp)
    assert_identical(got[0], got[1], got[2], oracle.sum, oracle.secondary, oracle.named(), "default")


# ---- render ------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", list(ms.SCENES))
def test_render_deform_reset_render(built, walk, kind):
    scene, camera, pos, idx, nrm = ms.SCENES[kind](RENDER_MESH, ASPECT)
    vp = viewport(scene, walk)
    passes(vp, camera, 2)
    last = vp.sum_buffer()
    walk_before = ra.update_info(vp.device_context())["walk"]
    if walk == "default":
        assert walk_before == {"two_level": "wide2", "single": "wide"}[kind]
    for step, with_normals in ((1, False), (2, True)):
        deform(scene, vp, pos, idx, step, with_normals)
        vp.reset()
        oracle = Oracle()
        passes(vp, camera, 2, oracle, scene)
        got = frame(vp)
        assert_identical(got[0], got[1], got[2], oracle.sum, oracle.secondary, oracle.named(), walk)
        assert not np.array_equal(got[0], last)          # the deformation shows
        last = got[0]
        info = ra.update_info(vp.device_context())
        assert info["walk"] == walk_before and info["numMeshUpdates"] == step
    # ray queries and one AOV call on the updated descriptor
    rays = shim.random_rays(scene, 8192, seed=9)
    hits, surf, _, _ = query_device(vp, ra.TRACE_CLOSEST, rays)
    ref_hits, ref_surf, _ = shim.closest(scene.desc, rays)
    assert (ref_hits[:, 1] != ra.RT_INVALID_OBJECT).mean() > 0.05
    assert np.array_equal(hits, ref_hits) and np.array_equal(surf, ref_surf)
    _, _, occ, _ = query_device(vp, ra.TRACE_ANY, rays)
    ref_occ, _ = shim.any_hit(scene.desc, rays)
    assert np.array_equal(occ, ref_occ) and 0.02 < ref_occ.mean() < 0.98
    # the AOV call: against a second context that takes the SAME updated descriptor whole (its own collapse, its own grid): the same first hits, word for word
    p = vp.next_pass_params(camera)
    planes = ("depth", "normal", "position", "object_id", "sub_object_id", "base_color")
    other = viewport(scene, walk)
    got, want = vp.render_aovs(p, planes), other.render_aovs(p, planes)
    for name in planes:
        assert np.array_equal(bits(got[name]), bits(want[name])), name
    on_mesh = np.isin(got["object_id"], mesh_objects(scene))
    assert on_mesh.sum() > 200
    # ... and the geometry planes against the first vertices of the oracle's paths on the updated descriptor, as tests/test_gpu_aovs.py holds them
    import aov_ref
    import path_records_ref
    flat_vp = ra.Viewport(W, H, seed=77, max_ray_depth=0)
    flat_vp.reset()
    p0 = flat_vp.next_pass_params(camera)
    assert p0.maxRayDepth == 0
    planes0 = vp.render_aovs(p0, aov_ref.GEOMETRY_PLANES)
    vertices = np.stack([oracle_lib.render_pixel_paths(scene.desc, p0, W, H, x, y, capacity=2)[0] for y in range(H) for x in range(W)])
    words, want = aov_ref.planes_as_vertex_words(planes0), vertices[:, 6:22].view(np.uint32)
    stale = np.concatenate([path_records_ref.stale_mask(vertices[i:i + 1], scene.desc.contents) for i in range(len(vertices))])[:, 6:22]
    differs = (words != want) & ~stale
    assert not differs.any(), int(differs.sum())
    assert not words[stale].any() and np.isin(planes0["object_id"], mesh_objects(scene)).sum() > 200


def test_vcm_photons_fall_at_the_update(built, walk):
    from test_gpu_update import VCM_ARGS, _vcm_viewport
    scene, camera, pos, idx, nrm = ms.two_level_scene(RENDER_MESH, ASPECT)
    vp = _vcm_viewport(scene, walk)
    for _ in range(2):
        vp.render_pass_with(vp.next_pass_params(camera))
    assert vp.vcm_num_photons() > 0
    deform(scene, vp, pos, idx, 1, True)
    assert vp.vcm_num_photons() == 0
    vp.reset()
    cam = np.zeros((H, W, 3), dtype=np.float32); cam2 = np.zeros((H, W, 3), dtype=np.float32); light = np.zeros((H, W, 3), dtype=np.float32)
    cnt = np.zeros(16, dtype=np.uint64)
    vcm = oracle_lib.Vcm(**VCM_ARGS)
    for i in range(2):
        p = vp.next_pass_params(camera)
        vp.render_pass_with(p)
        vcm.render_pass(scene.desc, p, W, H, cam, cam2 if i % 2 == 0 else None, light, cnt)
        assert vp.vcm_num_photons() == vcm.num_photons() > 0, i
    img, img2 = vp.sum_buffer(secondary=True)
    counters = vp.counters()
    assert np.array_equal(bits(img), bits(cam)), int(np.count_nonzero(bits(img) != bits(cam)))
    assert np.array_equal(bits(img2), bits(cam2))
    for n in (COMPARED if walk == "counting" else NOT_INTERSECTION):
        assert counters[n] == int(cnt[ra.COUNTER_NAMES.index(n)]), n


# ---- ordering ------------------------------------------------------------------------------------------------------------------------------------------
def test_passes_queued_before_the_update_show_the_old_mesh(built, walk):
    frames = []
    for synchronise in (False, True):
        scene, camera, pos, idx, nrm = ms.two_level_scene(RENDER_MESH, ASPECT)
        vp = viewport(scene, walk)
        oracle = Oracle()
        passes(vp, camera, 2, oracle, scene)
        if synchronise:
            vp.sum_buffer()
        deform(scene, vp, pos, idx, 1, True)
        passes(vp, camera, 2, oracle, scene)
        frames.append(frame(vp))
        assert_identical(frames[-1][0], frames[-1][1], frames[-1][2], oracle.sum, oracle.secondary, oracle.named(), walk)
    assert_same_frames(frames[0], frames[1], walk)


# ---- refusals ------------------------------------------------------------------------------------------------------------------------------------------
def test_a_refused_mesh_update_leaves_the_device_as_it_was(built, walk):
    lib = ra.rtgpu_lib()
    frames = []
    for refuse in (False, True):
        scene, camera, pos, idx, nrm = ms.two_level_scene(RENDER_MESH, ASPECT)
        vp = viewport(scene, walk)
        ctx = vp.device_context()
        new = np.ascontiguousarray(ms.deformed(pos, 1))
        mi = ms.mesh_index(scene)
        good = ra.RtMeshUpdate(3, mi, len(pos), 0, new.ctypes.data_as(C.POINTER(C.c_float)), None)
        assert good.abiVersion == lib.rtgpu_abi_version()
        if refuse:
            assert lib.rtgpu_update_mesh(ctx, C.byref(good)) == NOT_READY                     # nothing uploaded yet
        vp.update_scene()
        if refuse:
            nan = new.copy(); nan[len(nan) // 2, 1] = np.nan
            inf = new.copy(); inf[0, 0] = np.inf
            bad = [ra.RtMeshUpdate(3, mi, len(pos) - 1, 0, good.positions, None), ra.RtMeshUpdate(3, mi, len(pos), 0, nan.ctypes.data_as(C.POINTER(C.c_float)), None),
                   ra.RtMeshUpdate(3, mi, len(pos), 0, inf.ctypes.data_as(C.POINTER(C.c_float)), None), ra.RtMeshUpdate(3, 2, len(pos), 0, good.positions, None),
                   ra.RtMeshUpdate(3, mi, len(pos), 0, None, None), ra.RtMeshUpdate(2, mi, len(pos), 0, good.positions, None), ra.RtMeshUpdate(3, mi, len(pos), 1, good.positions, None),
                   ra.RtMeshUpdate(3, 1 - mi, len(pos), 0, good.positions, None)]      # (the last: the prop's mesh, which has another vertex count)
            for u in bad:
                assert lib.rtgpu_update_mesh(ctx, C.byref(u)) == INVALID_ARGUMENT, lib.rtgpu_last_error()
            # positions whose box the 16-bit grid cannot hold with its margin -- the sheet settled flat at z = 0.25, the mesh far from its origin --: an upload
            # leaves such a mesh to the binary walk, an update refuses before it writes (the scene has 4-wide tables under either walk)
            flat, far = np.ascontiguousarray(flattened(new)), np.ascontiguousarray(new + np.float32(1.0e4))
            for positions in (flat, far):
                u = ra.RtMeshUpdate(3, mi, len(pos), 0, positions.ctypes.data_as(C.POINTER(C.c_float)), None)
                assert lib.rtgpu_update_mesh(ctx, C.byref(u)) == UNSUPPORTED and b"grid" in lib.rtgpu_last_error(), lib.rtgpu_last_error()
            assert lib.rtgpu_update_mesh(ctx, None) == INVALID_ARGUMENT and lib.rtgpu_update_mesh(None, C.byref(good)) == INVALID_ARGUMENT
            assert ra.update_info(ctx)["numMeshUpdates"] == 0
        oracle = Oracle()
        passes(vp, camera, 2, oracle, scene)
        frames.append(frame(vp))
        assert_identical(frames[-1][0], frames[-1][1], frames[-1][2], oracle.sum, oracle.secondary, oracle.named(), walk)
    assert_same_frames(frames[1], frames[0], walk)       # bit-identical to a context that never saw the calls
    # and the update itself, unbroken, is taken (the mirror follows: the oracle's descriptor is the refit scene)
    assert lib.rtgpu_update_mesh(ctx, C.byref(good)) == OK, lib.rtgpu_last_error()
    assert ra.update_info(ctx)["numMeshUpdates"] == 1
    scene.set_mesh_vertices(ms.MESH_OBJECT, new)
    scene.update()
    vp.update_scene()            # (the mirror sends the same positions once more, and the top level over the new boxes)
    vp.reset()
    oracle = Oracle()
    passes(vp, camera, 2, oracle, scene)
    got = frame(vp)
    assert_identical(got[0], got[1], got[2], oracle.sum, oracle.secondary, oracle.named(), walk)


# ---- temporal ------------------------------------------------------------------------------------------------------------------------------------------
GUIDES = ("depth", "normal", "position", "base_color", "object_id")


@pytest.mark.parametrize("clip", [None, dict(radius=3, gamma=1.0, min_count=9)], ids=["plain", "clip"])
def test_the_history_survives_a_mesh_update_except_on_the_mesh(built, clip):
    """frame 0 stores a history; the mesh deforms; frame 1's call is the model under the table of the header: prevId 0xFFFFFFFF for the mesh's objects (their
    pixels start: history length 1), the identity for all others (they reproject as before)"""
    scene, camera, pos, idx, nrm = ms.two_level_scene(RENDER_MESH, ASPECT)
    scene.desc.contents.blueNoise = BLUE_NOISE.ctypes.data
    vp = ra.Viewport(W, H, seed=2468, max_ray_depth=3)
    vp.set_renderer(scene)
    history, prev = None, None
    for k in range(3):
        if k:
            deform(scene, vp, pos, idx, k, True)
        vp.reset()
        params = [vp.next_pass_params(camera) for _ in range(3)]
        for p in params[:2]:
            vp.render_pass_with(p)
        s, s2 = vp.sum_buffer(secondary=True)
        g = vp.render_aovs(params[2], GUIDES)
        image = vp.denoise(params[2], temporal=True, variance=False, clip=clip)
        accumulate, accumulate_moving = temporal_ref.accumulate, mref.accumulate_moving
        if clip is not None:
            import temporal_clip_ref as cref
            accumulate = accumulate_moving = lambda **a: cref.accumulate_clip(clip=clip, **a)[:4]       # (the clipped model takes the table, or none, itself)
        kw = dict(color=s, color_half=s2, depth=g["depth"], normal=g["normal"], position=g["position"], albedo=g["base_color"], object_id=g["object_id"], history=history,
                  color_scale=0.5)
        if history is None:
            new_history, _, _, why = accumulate(**kw)
        else:
            kw.update(prev_world_to_screen=list(prev.camera.worldToScreen), prev_sample_offset=tuple(prev.sampleOffset))
            n = scene.desc.contents.numObjects
            u = scene.update_desc()                  # (the top level was rebuilt over the new boxes: current object i was previousIndex[i] when the history was stored)
            prev_ids = np.array([u.previousIndex[i] for i in range(n)], dtype=np.uint32)
            prev_ids[mesh_objects(scene)] = 0xFFFFFFFF
            table = (np.tile(np.eye(4, dtype=np.float32), (n, 1, 1)), prev_ids, np.zeros(n, dtype=np.uint32))
            new_history, _, _, why = accumulate_moving(object_motion=table, **kw)
            on_mesh = np.isin(g["object_id"], mesh_objects(scene))
            assert on_mesh.sum() > 200 and (new_history["length"][on_mesh] == 1).all()
            others = ~on_mesh & np.isfinite(g["depth"])
            assert (why[others] == temporal_ref.BLENDED).mean() > 0.5 and (new_history["length"][others] > 1).mean() > 0.5       # everything else keeps its history
        want = temporal_ref.remodulate(new_history["a"], g["base_color"])
        assert np.array_equal(bits(image), bits(want)), (k, int(np.count_nonzero(bits(image) != bits(want))))
        history, prev = new_history, params[2]


# ---- several devices -----------------------------------------------------------------------------------------------------------------------------------
def test_the_mesh_update_reaches_both_peers(built):
    """one device used as two (the one-device leg tests/test_gpu_multi_device.py offers): the update goes to both contexts; never run on two physical devices"""
    frames, params = [], None
    for devices in (None, [0, 0]):
        scene, camera, pos, idx, nrm = ms.two_level_scene(RENDER_MESH, ASPECT)
        vp = viewport(scene, "default", devices=devices)
        passes(vp, camera, 1)
        deform(scene, vp, pos, idx, 1, True)
        vp.reset()
        if params is None:
            params = passes(vp, camera, 2)
        else:
            for p in params:
                vp.render_pass_with(p)
        frames.append(frame(vp))
    assert ra.multi_info(vp.device_context())["numDevices"] == 2
    assert_same_frames(frames[1], frames[0], "default")


def test_the_mesh_update_on_two_physical_devices(built):
    """the same over devices 0 and 1; skips on a box with one device (this leg has never run)"""
    import torch
    if torch.cuda.device_count() < 2:
        pytest.skip("one device on this box")
    frames, params = [], None
    for devices in (None, [0, 1]):
        scene, camera, pos, idx, nrm = ms.two_level_scene(RENDER_MESH, ASPECT)
        vp = viewport(scene, "default", devices=devices)
        passes(vp, camera, 1)
        deform(scene, vp, pos, idx, 1, True)
        vp.reset()
        if params is None:
            params = passes(vp, camera, 2)
        else:
            for p in params:
                vp.render_pass_with(p)
        frames.append(frame(vp))
    assert ra.multi_info(vp.device_context())["numDevices"] == 2
    assert_same_frames(frames[1], frames[0], "default")
