"""Beam lists on the GPU (include/rtgpu.h: rtgpu_get_beam_list_info; raytracer_amd/csrc/rt_beam_lists.h, rt_trace_packet.inl): a still camera's packets take
their leaves from per-tile lists, and nothing but numRetracedRays may show it.  64 x 48 unless said, depth 4, 8 passes in batches of two: the first batch meets
no camera before it, the second builds, the third and fourth scan.  Every comparison is on bits."""
import ctypes as C

import numpy as np
import pytest

import oracle_lib
import raytracer_amd as ra

import beam_scenes

pytestmark = pytest.mark.gpu

W, H, DEPTH, PASSES, SEED, SPREAD = 64, 48, 4, 8, 7, 0.5
REFERENCE_COUNTERS = ("numRays", "numPrimaryRays", "numShadowRays", "numShadowRaysHit", "numMeshHits", "numAnalyticHits")
NO_LIST = 0xFFFFFFFF


@pytest.fixture(autouse=True)
def batches_of_two(monkeypatch):
    monkeypatch.setenv("RTGPU_PASS_BATCH", "2")


def viewport(scene, w=W, h=H, spread=SPREAD, seed=SEED):
    scene.desc.contents.blueNoise = ra.load_blue_noise().ctypes.data
    vp = ra.Viewport(w, h, seed=seed, max_ray_depth=DEPTH, anti_aliasing_spread=spread)
    vp.set_renderer(scene)
    return vp


def passes_of(vp, camera, n=PASSES):
    out = []
    for _ in range(n):
        p = vp.next_pass_params(camera)
        vp.render_pass_with(p)
        out.append(p)
    return out


def frame(vp):
    img, img2 = vp.sum_buffer(secondary=True)
    c = vp.counters()
    return img, img2, {n: c[n] for n in REFERENCE_COUNTERS}


def same(a, b):
    assert np.array_equal(a[0].view(np.uint32), b[0].view(np.uint32)), "%d sum-buffer words differ" % np.count_nonzero(a[0].view(np.uint32) != b[0].view(np.uint32))
    assert np.array_equal(a[1].view(np.uint32), b[1].view(np.uint32))
    assert a[2] == b[2]


def oracle_frame(scene, params, w=W, h=H, shard=None):
    ref, ref2, cnt = np.zeros((h, w, 3), dtype=np.float32), np.zeros((h, w, 3), dtype=np.float32), np.zeros(16, dtype=np.uint64)
    for p in params:
        if shard is None:
            oracle_lib.render_pass(scene.desc, p, w, h, ref, ref2, cnt, threads=8)
        else:
            oracle_lib.render_pass(scene.desc, p, w, h, ref, ref2, cnt, shard=shard, threads=8)
    return ref, ref2, {n: int(cnt[i]) for i, n in enumerate(ra.COUNTER_NAMES) if n in REFERENCE_COUNTERS}


def share_scanned(info):
    total = info["packetsScanned"] + info["packetsWalkedOffset"] + info["packetsWalkedNoList"]
    return info["packetsScanned"] / max(1, total)


def on_and_off(monkeypatch, make, w=W, h=H, spread=SPREAD, setup=None, n=PASSES):
    """The same render with the lists on and with RTGPU_BEAM_LISTS=0: (scene, params, on frame, on info, off frame)."""
    legs = []
    for lists in ("1", "0"):
        monkeypatch.setenv("RTGPU_BEAM_LISTS", lists)
        scene, camera = make(w / h)
        vp = viewport(scene, w, h, spread)
        if setup:
            setup(vp)
        params = passes_of(vp, camera, n)
        legs.append((scene, params, frame(vp), vp.beam_list_info(), vp))
    monkeypatch.setenv("RTGPU_BEAM_LISTS", "1")
    assert legs[1][3]["builds"] == 0 and legs[1][3]["packetsScanned"] == 0
    return legs[0][0], legs[0][1], legs[0][2], legs[0][3], legs[1][2], legs[0][4]


def building(aspect):
    return beam_scenes.mesh_scene(aspect, 2000)


def test_a_lists_on_equal_lists_off_and_the_oracle(built, monkeypatch):
    """The room: at 64 x 48 a tile of the 2000-triangle building spans up to a hundred leaves and some tiles overflow 64 entries (the host builder says so, below the
    share is a condition); the room's twelve triangles never do."""
    scene, params, on, info, off, vp = on_and_off(monkeypatch, beam_scenes.box_room)
    # the preconditions of the share below, on the CPU: every pass's offset lies within m, and the host builder leaves no tile of this scene without a list
    assert all(abs(p.sampleOffset[0]) <= 3 * SPREAD and abs(p.sampleOffset[1]) <= 3 * SPREAD for p in params)
    host_counts, _ = vp.beam_lists(from_host=True)
    assert info["numTiles"] == W * H // 64 and not np.any(host_counts == NO_LIST)
    same(on, off)
    same(on, oracle_frame(scene, params))
    assert info["builds"] == 1 and info["valid"] == 1 and info["margin"] == pytest.approx(3 * SPREAD)
    # three batches of two passes behind the build, 48 packets a pass; a condition, not a measurement: the test must not pass on the fallback
    assert info["packetsScanned"] + info["packetsWalkedOffset"] + info["packetsWalkedNoList"] == 3 * 2 * (W * H // 64)
    assert share_scanned(info) >= 0.9, info


def test_a_the_building_with_some_tiles_over_the_capacity(built, monkeypatch):
    scene, params, on, info, off, vp = on_and_off(monkeypatch, building)
    same(on, off)
    same(on, oracle_frame(scene, params))
    counts, _ = vp.beam_lists(from_host=True)
    listed = int(np.count_nonzero(counts != NO_LIST))
    assert info["builds"] == 1 and 0 < listed and info["packetsScanned"] == 3 * 2 * listed and info["packetsWalkedNoList"] == 3 * 2 * (len(counts) - listed), info


def test_b_passes_whose_offset_exceeds_the_margin_walk(built, monkeypatch):
    """antiAliasingSpread 2 under a margin held at 1.5 pixels: most passes' offsets exceed it."""
    scene, params, on, info, off, _ = on_and_off(monkeypatch, building, spread=2.0, setup=lambda vp: vp.set_beam_margin(1.5))
    beyond = [abs(p.sampleOffset[0]) > 1.5 or abs(p.sampleOffset[1]) > 1.5 for p in params]
    assert any(beyond[2:]), "pick another seed: no pass behind the build exceeds the margin"
    same(on, off)
    assert info["margin"] == 1.5 and info["packetsWalkedOffset"] == sum(beyond[2:]) * (W * H // 64), (info, beyond)
    assert info["packetsScanned"] + info["packetsWalkedNoList"] == (len(beyond[2:]) - sum(beyond[2:])) * (W * H // 64) and info["packetsScanned"] > 0


def test_c_a_capacity_of_two_leaves_most_tiles_without_a_list(built, monkeypatch):
    monkeypatch.setenv("RTGPU_BEAM_LIST_CAP", "2")
    scene, params, on, info, off, _ = on_and_off(monkeypatch, building)
    same(on, off)
    assert info["builds"] == 1 and info["capacity"] == 2 and info["packetsWalkedNoList"] > info["packetsScanned"], info


@pytest.mark.parametrize("shard", [None, (0, 2)])
def test_d_partial_tiles_and_a_shard(built, monkeypatch, shard):
    w, h = 60, 44
    scene, params, on, info, off, _ = on_and_off(monkeypatch, building, w, h, setup=(lambda vp: vp.set_shard(*shard)) if shard else None)
    same(on, off)
    same(on, oracle_frame(scene, params, w, h, shard=shard))
    assert info["builds"] == 1 and info["packetsScanned"] > 0, info


def test_e_a_rigid_transform_uses_lists_and_a_scaled_object_builds_none(built, monkeypatch):
    scene, params, on, info, off, _ = on_and_off(monkeypatch, lambda a: beam_scenes.mesh_scene(a, 2000, beam_scenes.RIGID))
    same(on, off)
    same(on, oracle_frame(scene, params))
    assert info["builds"] == 1 and info["packetsScanned"] > 0, info
    scaled = (C.c_float * 16)(*beam_scenes.RIGID)
    for k in range(12):
        scaled[k] *= 1.5
    scene, params, on, info, off, _ = on_and_off(monkeypatch, lambda a: beam_scenes.mesh_scene(a, 2000, scaled))
    same(on, off)
    assert info["builds"] == 0 and info["valid"] == 0, info


def _dof(aspect):
    scene, camera = building(aspect)
    camera.set_dof(True, 6.0, 0.05)
    return scene, camera


def _barrel(aspect):
    scene, camera = building(aspect)
    camera.set_lens(0, 0.01, 0.05)
    return scene, camera


@pytest.mark.parametrize("make", [_dof, _barrel], ids=["dof", "barrel"])
def test_f_other_cameras_build_no_lists(built, monkeypatch, make):
    scene, params, on, info, off, _ = on_and_off(monkeypatch, make)
    same(on, off)
    same(on, oracle_frame(scene, params))
    assert info["builds"] == 0 and info["packetsScanned"] == 0, info


@pytest.mark.parametrize("kind", ["rays", "lens"])
def test_f_a_ray_or_lens_source_builds_no_lists(built, monkeypatch, kind):
    def source(vp):
        scene_camera = building(W / H)[1]
        p = ra.Viewport(W, H, seed=3, anti_aliasing_spread=0.0).next_pass_params(scene_camera)
        if kind == "rays":
            vp.set_ray_source(vp.camera_rays(p))
        else:
            vp.set_lens_source(vp.camera_footprints(p))
    scene, params, on, info, off, _ = on_and_off(monkeypatch, building, setup=source)
    same(on, off)
    assert info["builds"] == 0 and info["packetsScanned"] == 0, info


def _two_renders(monkeypatch, between, second_size=None):
    """One context: 4 passes, `between(vp, scene, camera)` -> the camera to go on with, 6 passes more; then the second render alone in a fresh context."""
    scene, camera = building(W / H)
    vp = viewport(scene)
    passes_of(vp, camera, 4)
    before = vp.beam_list_info()
    camera2 = between(vp, scene, camera) or camera
    w, h = second_size or (W, H)
    vp.reset()
    params = passes_of(vp, camera2, 6)
    again = frame(vp)
    after = vp.beam_list_info()
    fresh = ra.Viewport(w, h, seed=SEED, max_ray_depth=DEPTH, anti_aliasing_spread=SPREAD)
    fresh.set_renderer(scene)
    for p in params:
        fresh.render_pass_with(p)
    same(again, frame(fresh))
    assert before["builds"] == 1 and after["builds"] == 2 and after["packetsScanned"] > before["packetsScanned"], (before, after)


def test_g_a_changed_camera_rebuilds(built, monkeypatch):
    _two_renders(monkeypatch, lambda vp, scene, camera: ra.Camera((-11.0, 2.6, 0.2), (2.0, 70.0, 0.0), W / H, 65.0))


def test_g_an_object_update_rebuilds(built, monkeypatch):
    def move(vp, scene, camera):
        scene.set_object_transform(0, beam_scenes.RIGID)
        scene.update()
        vp.update_scene()
    _two_renders(monkeypatch, move)


def test_g_a_mesh_update_rebuilds(built, monkeypatch):
    def deform(vp, scene, camera):
        pos = next(args for kind, args in scene.calls if kind == "mesh")["positions"].copy()
        pos[:, 1] *= np.float32(1.05)
        scene.set_mesh_vertices(0, pos)
        scene.update()
        vp.update_scene()
    _two_renders(monkeypatch, deform)


def test_g_a_resize_rebuilds(built, monkeypatch):
    scene, camera = building(W / H)
    vp = viewport(scene)
    passes_of(vp, camera, 4)
    before = vp.beam_list_info()
    assert ra.rtgpu_lib().rtgpu_resize(vp.device_context(), 60, 44) == 0 and ra.rtgpu_lib().rtgpu_resize(vp.device_context(), W, H) == 0
    vp.reset()
    params = passes_of(vp, camera, 6)
    again, after = frame(vp), vp.beam_list_info()
    fresh = viewport(scene)
    for p in params:
        fresh.render_pass_with(p)
    same(again, frame(fresh))
    assert before["builds"] == 1 and after["builds"] == 2, (before, after)


@pytest.mark.parametrize("cap", [64, 2])
def test_h_device_lists_are_the_host_builder_s(built, monkeypatch, cap):
    monkeypatch.setenv("RTGPU_BEAM_LIST_CAP", str(cap))
    for make, size in ((building, (W, H)), (building, (60, 44)), (beam_scenes.box_room, (W, H))):
        scene, camera = make(size[0] / size[1])
        vp = viewport(scene, *size)
        passes_of(vp, camera, 4)
        dev_counts, dev_entries = vp.beam_lists()
        host_counts, host_entries = vp.beam_lists(from_host=True)
        assert np.array_equal(dev_counts, host_counts)
        assert cap == 2 or np.any(dev_counts != NO_LIST)   # (at two entries a small frame of the building keeps no list at all)
        for t in np.nonzero(dev_counts != NO_LIST)[0]:
            n = dev_counts[t]
            assert set(map(tuple, dev_entries[t, :n])) == set(map(tuple, host_entries[t, :n])), t
            assert np.all(np.diff(dev_entries[t, :n, 1].view(np.float32)) >= 0)


def _cameras(n):
    return [ra.Camera((-12.5 + 0.3 * k, 2.2 + 0.1 * k, 0.6), (4.0, 82.0 - 3.0 * k, 0.0), W / H, 65.0) for k in range(n)]


def test_a_camera_that_moves_with_every_batch_never_builds(built, monkeypatch):
    scene, _ = building(W / H)
    vp = viewport(scene)
    for camera in _cameras(5):
        passes_of(vp, camera, 2)     # one batch per camera
    info = vp.beam_list_info()
    assert info["builds"] == 0 and info["allocations"] == 0 and info["valid"] == 0 and info["packetsScanned"] == 0, info


def test_rebuilds_keep_the_device_arrays_bounded(built, monkeypatch):
    """A camera that rests for two batches and moves on, eight times over.  With a synchronising call between the rests every rebuild rewrites the one set of
    arrays in place; without one, arrays that launches in flight may read are retired, at most four of them, and the frame is the walk's."""
    two = _cameras(2)
    scene, _ = building(W / H)
    vp = viewport(scene)
    for k in range(8):
        passes_of(vp, two[k & 1], 4)
        info = vp.beam_list_info()   # synchronises
        assert info["builds"] == k + 1 and info["allocations"] == 1 and info["retiredArrays"] == 0, (k, info)
    frames = []
    for lists in ("1", "0"):
        monkeypatch.setenv("RTGPU_BEAM_LISTS", lists)
        scene, _ = building(W / H)
        vp = viewport(scene)
        for k in range(8):
            passes_of(vp, two[k & 1], 4)
        info = vp.beam_list_info()   # the first synchronising call
        frames.append(frame(vp))
        if lists == "1":
            assert info["builds"] == 8 and 1 <= info["allocations"] <= 8 and info["retiredArrays"] <= 4 and info["packetsScanned"] > 0, info
            assert vp.beam_list_info()["retiredArrays"] == 0
    same(frames[0], frames[1])
