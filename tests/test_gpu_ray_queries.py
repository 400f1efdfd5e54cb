"""Batched ray queries on the device (include/rtgpu.h: rtgpu_trace_rays / rtgpu_trace_rays_async, Viewport.trace_rays / occluded) held bit for
bit to the oracle's scene walk (tests/cpp/ray_query_oracle.cpp, itself pinned to the reference by tests/test_ray_queries_cpu.py), on the walk the
context renders with: "default" = the 4-wide walks and their re-trace hand-over, "counting" = the reference's binary walk with its box / triangle
test counters, which must equal the oracle's."""
import ctypes as C

import numpy as np
import pytest

import kat_io
import ray_query_shim as shim
import raytracer_amd as ra
import scene_zoo
from raytracer_amd import scenes
from test_ray_queries_cpu import check_mesh_kat

SCENES = {
    "cornell_box": lambda: scenes.cornell_box(4 / 3)[0],
    "mesh_scene": lambda: scene_zoo.mesh_scene(4 / 3)[0],
    "textured_scene": lambda: scene_zoo.textured_scene(4 / 3)[0],
    "sponza_class": lambda: scenes.sponza_class(16 / 9)[0],
    "random_3": lambda: scene_zoo.random_scene(4 / 3, 3)[0],
    "random_17": lambda: scene_zoo.random_scene(4 / 3, 17)[0],
    "random_42": lambda: scene_zoo.random_scene(4 / 3, 42)[0],
}
NUM_RAYS = 65536
CLOSEST_TESTS = ("numRayBoxTests", "numPassedRayBoxTests", "numRayTriangleTests", "numPassedRayTriangleTests")
ANY_TESTS = ("numShadowRayBoxTests", "numShadowRayTriangleTests")
FIELD = {n: i for i, (n, _) in enumerate(ra.RtCounters._fields_)}


def viewport(scene, walk="default", **kw):
    vp = ra.Viewport(32, 24, seed=5)
    vp.set_renderer(scene, intersection_counters=(walk == "counting"), **kw)
    assert ra.host_lib().rth_viewport_upload_scene(vp._h) == 0   # (the raw C calls below; Viewport.trace_rays does this itself)
    return vp


def device(vp, mode, rays, surfaces=True):
    """the host entry point on raw records: (hits, surfaces, occluded, stats)"""
    lib = ra.rtgpu_lib()
    n = len(rays)
    hits = np.zeros((n, 8), dtype=np.uint32) if mode == ra.TRACE_CLOSEST else None
    surf = np.zeros((n, 12), dtype=np.uint32) if (surfaces and mode == ra.TRACE_CLOSEST) else None
    occ = np.zeros(n, dtype=np.uint32) if mode == ra.TRACE_ANY else None
    stats = ra.RtCounters()
    p = lambda a: a.ctypes.data_as(C.c_void_p) if a is not None else None   # noqa: E731
    r = lib.rtgpu_trace_rays(vp.device_context(), C.c_uint32(mode), p(np.ascontiguousarray(rays)), C.c_uint32(n), p(hits), p(surf), p(occ), C.byref(stats))
    assert r == 0, lib.rtgpu_last_error()
    return hits, surf, occ, np.array([getattr(stats, f) for f, _ in ra.RtCounters._fields_[:13]], dtype=np.uint64)


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(SCENES))
def test_device_queries_equal_the_oracle_walk(built, walk, name):
    scene = SCENES[name]()
    rays = shim.random_rays(scene, NUM_RAYS, seed=sorted(SCENES).index(name) + 1)
    vp = viewport(scene, walk)
    hits, surf, _, stats = device(vp, ra.TRACE_CLOSEST, rays)
    ref_hits, ref_surf, ref_cnt = shim.closest(scene.desc, rays)
    assert (ref_hits[:, 1] != ra.RT_INVALID_OBJECT).mean() > 0.05
    bad = np.nonzero((hits != ref_hits).any(axis=1))[0]
    assert len(bad) == 0, (name, walk, bad[:8].tolist(), hits[bad[:2]].tolist(), ref_hits[bad[:2]].tolist(), rays[bad[:2]].tolist())
    bad = np.nonzero((surf != ref_surf).any(axis=1))[0]
    assert len(bad) == 0, (name, walk, bad[:8].tolist(), surf[bad[:2]].tolist(), ref_surf[bad[:2]].tolist())
    _, _, occ, any_stats = device(vp, ra.TRACE_ANY, rays)
    ref_occ, ref_any = shim.any_hit(scene.desc, rays)
    assert 0.05 < ref_occ.mean() < 0.95
    bad = np.nonzero(occ != ref_occ)[0]
    assert len(bad) == 0, (name, walk, len(bad), bad[:8].tolist(), occ[bad[:8]].tolist(), rays[bad[:4]].tolist())
    if walk == "counting":
        # closest-hit rays are walked from +inf and maxDistance applied to the record (include/rtgpu.h): their test counts are those of that walk
        unbounded = rays.copy()
        unbounded[:, 3] = shim.INF
        _, _, ref_cnt = shim.closest(scene.desc, unbounded, surfaces=False)
        for f in CLOSEST_TESTS:
            assert stats[FIELD[f]] == ref_cnt[FIELD[f]], f
        for f in ANY_TESTS:
            assert any_stats[FIELD[f]] == ref_any[FIELD[f]], f
        assert stats[FIELD["numRays"]] == ref_cnt[FIELD["numRays"]]


@pytest.mark.gpu
def test_mesh_kat_through_the_public_call(built, walk):
    scene, _, _ = kat_io.mesh_fixture_scene()
    kat_rays, _, _ = shim.mesh_kat()
    rays = shim.kat_query_rays(kat_rays)
    vp = viewport(scene, walk)
    hits, surf, _, _ = device(vp, ra.TRACE_CLOSEST, rays)
    _, _, occ, _ = device(vp, ra.TRACE_ANY, rays)
    check_mesh_kat(hits, surf, occ)
    # and the Python surface returns the same records
    res = vp.trace_rays(kat_rays[:, 0:3].copy(), kat_rays[:, 3:6].copy(), kat_rays[:, 6].copy(), surfaces=True)
    assert np.array_equal(res.distance.view(np.uint32), hits[:, 0]) and np.array_equal(res.object_id, hits[:, 1])
    assert np.array_equal(res.uv.view(np.uint32), hits[:, 3:5]) and np.array_equal(res.material, surf[:, 11])
    assert np.array_equal(vp.occluded(kat_rays[:, 0:3].copy(), kat_rays[:, 3:6].copy(), kat_rays[:, 6].copy()), occ != 0)


@pytest.mark.gpu
def test_torch_tensors_on_the_current_stream(built, walk):
    import torch
    scene = SCENES["mesh_scene"]()
    rays = shim.random_rays(scene, NUM_RAYS, seed=99)
    vp = viewport(scene, walk)
    host = vp.trace_rays(rays[:, 0:3].copy(), rays[:, 4:7].copy(), rays[:, 3].copy(), surfaces=True)
    host_occ = vp.occluded(rays[:, 0:3].copy(), rays[:, 4:7].copy(), rays[:, 3].copy())
    base = torch.from_numpy(rays).to("cuda:0")
    # produced by kernels on the current stream right before the calls, no synchronisation in between
    origins = (base[:, 0:3] * 1.0).contiguous()
    directions = (base[:, 4:7] + 0.0).contiguous()
    max_distance = base[:, 3] * 1.0
    dev = vp.trace_rays(origins, directions, max_distance, surfaces=True)
    dev_occ = vp.occluded(origins, directions, max_distance)
    torch.cuda.synchronize()
    assert dev.distance.device.type == "cuda" and dev_occ.dtype == torch.bool
    for k in host._fields:
        a, b = getattr(host, k), getattr(dev, k).cpu().numpy()
        if a.dtype == np.float32:
            assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), k
        else:
            assert np.array_equal(a.astype(np.int64), b), k
    assert np.array_equal(host_occ, dev_occ.cpu().numpy())


@pytest.mark.gpu
def test_chunked_call_equals_its_chunks(built):
    scene = SCENES["cornell_box"]()
    chunk = 1 << 22
    rng = np.random.RandomState(3)
    n = chunk + 5000
    lo, hi = shim.scene_bounds(scene)
    o = (lo + rng.rand(n, 3) * (hi - lo)).astype(np.float32)
    d = rng.normal(size=(n, 3)).astype(np.float32)
    vp = viewport(scene)
    whole = vp.trace_rays(o, d, surfaces=True)
    first = vp.trace_rays(o[:chunk].copy(), d[:chunk].copy(), surfaces=True)
    second = vp.trace_rays(o[chunk:].copy(), d[chunk:].copy(), surfaces=True)
    for k in whole._fields:
        assert np.array_equal(np.concatenate([getattr(first, k), getattr(second, k)]).view(np.uint32), getattr(whole, k).view(np.uint32)), k
    occ = vp.occluded(o, d)
    assert np.array_equal(np.concatenate([vp.occluded(o[:chunk].copy(), d[:chunk].copy()), vp.occluded(o[chunk:].copy(), d[chunk:].copy())]), occ)


@pytest.mark.gpu
def test_error_codes_and_degenerate_rays(built):
    import torch
    lib = ra.rtgpu_lib()
    scene = SCENES["mesh_scene"]()
    vp = viewport(scene)
    ctx = vp.device_context()
    rays = shim.random_rays(scene, 4096, seed=7)
    hits = np.zeros((4096, 8), dtype=np.uint32)
    occ = np.zeros(4096, dtype=np.uint32)
    P = lambda a: a.ctypes.data_as(C.c_void_p)   # noqa: E731
    assert lib.rtgpu_trace_rays(ctx, 0, None, 0, None, None, None, None) == 0                       # count 0: no-op
    assert lib.rtgpu_trace_rays(ctx, 0, None, 16, P(hits), None, None, None) == -1                  # NULL rays
    assert lib.rtgpu_trace_rays(ctx, 0, P(rays), 16, None, None, None, None) == -1                  # NULL hits
    assert lib.rtgpu_trace_rays(ctx, 7, P(rays), 16, P(hits), None, None, None) == -1               # unknown mode
    assert lib.rtgpu_trace_rays(ctx, 1, P(rays), 16, P(hits), None, P(occ), None) == -1             # hits in any mode
    assert lib.rtgpu_trace_rays(ctx, 1, P(rays), 16, None, P(hits), P(occ), None) == -1             # surfaces in any mode
    assert lib.rtgpu_trace_rays(ctx, 0, P(rays), 16, P(hits), None, P(occ), None) == -1             # occluded in closest mode
    fresh = C.c_void_p()
    assert lib.rtgpu_create(0, C.byref(fresh)) == 0
    try:
        assert lib.rtgpu_trace_rays(fresh, 0, P(rays), 16, P(hits), None, None, None) == -5         # no scene
        assert lib.rtgpu_trace_rays_async(fresh, 0, P(rays), 16, P(hits), None, None, None, None) == -5
    finally:
        lib.rtgpu_destroy(fresh)
    bad = rays.copy()
    degenerate = [(0, 1, np.nan), (1, 5, np.nan), (2, 0, np.inf), (3, 3, 0.0), (4, 3, np.nan), (5, 6, np.inf)]   # (ray, word, value): 0-2 origin, 3 maxDistance, 4-6 direction
    for i, w, val in degenerate:
        bad[i, w] = val
    bad[6, 4:7] = 0.0
    bad[7, 4:7] = 1e-30   # squared length underflows to 0
    with pytest.raises(ValueError):   # the host entry point refuses them
        vp.trace_rays(bad[:, 0:3].copy(), bad[:, 4:7].copy(), bad[:, 3].copy())
    t = torch.from_numpy(bad).to("cuda:0")
    res = vp.trace_rays(t[:, 0:3].contiguous(), t[:, 4:7].contiguous(), t[:, 3].contiguous(), surfaces=True)
    occ_dev = vp.occluded(t[:, 0:3].contiguous(), t[:, 4:7].contiguous(), t[:, 3].contiguous())
    torch.cuda.synchronize()
    ids = res.object_id.cpu().numpy()
    assert np.all(ids[:8] == ra.RT_INVALID_OBJECT) and not occ_dev[:8].any()
    assert np.all(res.material.cpu().numpy()[:8] == ra.RT_NO_MATERIAL)
    ref_hits, ref_surf, _ = shim.closest(scene.desc, bad)
    ref_occ, _ = shim.any_hit(scene.desc, bad)
    assert np.array_equal(res.distance.cpu().numpy().view(np.uint32)[8:], ref_hits[8:, 0])
    assert np.array_equal(ids[8:].astype(np.uint32), ref_hits[8:, 1])
    assert np.array_equal(res.position.cpu().numpy().view(np.uint32)[8:], ref_surf[8:, 0:3])
    assert np.array_equal(occ_dev.cpu().numpy()[8:], ref_occ[8:] != 0)


@pytest.mark.gpu
def test_queries_leave_the_render_alone(built):
    scene, camera = scenes.cornell_box(4 / 3)
    rays = shim.random_rays(scene, 20000, seed=12)
    o, d, m = rays[:, 0:3].copy(), rays[:, 4:7].copy(), rays[:, 3].copy()

    def run(with_queries):
        vp = ra.Viewport(64, 48, seed=77, max_ray_depth=5)
        vp.set_renderer(scene)
        answers = []
        for _ in range(4):
            vp.render(camera, passes=1)
            if with_queries:
                answers.append((vp.trace_rays(o, d, m, surfaces=True).distance, vp.occluded(o, d, m)))
        if with_queries:
            answers.append((vp.trace_rays(o, d, m, surfaces=True).distance, vp.occluded(o, d, m)))
        s, s2 = vp.sum_buffer(secondary=True)
        return s, s2, vp.counters(), answers
    s_a, s2_a, c_a, answers = run(True)
    s_b, s2_b, c_b, _ = run(False)
    assert np.array_equal(s_a.view(np.uint32), s_b.view(np.uint32))
    assert np.array_equal(s2_a.view(np.uint32), s2_b.view(np.uint32))
    assert c_a == c_b
    for dist, occ in answers[1:]:
        assert np.array_equal(dist.view(np.uint32), answers[0][0].view(np.uint32)) and np.array_equal(occ, answers[0][1])


@pytest.mark.gpu
def test_multi_device_context_answers_like_one_device(built, walk):
    scene = SCENES["random_17"]()
    rays = shim.random_rays(scene, 16384, seed=4)
    one = device(viewport(scene, walk), ra.TRACE_CLOSEST, rays)
    multi_vp = viewport(scene, walk, devices=[0])
    multi = device(multi_vp, ra.TRACE_CLOSEST, rays)
    assert np.array_equal(one[0], multi[0]) and np.array_equal(one[1], multi[1])
    assert np.array_equal(device(viewport(scene, walk), ra.TRACE_ANY, rays)[2], device(multi_vp, ra.TRACE_ANY, rays)[2])
