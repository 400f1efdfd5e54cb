"""The ray queries of include/rtgpu.h (rtgpu_trace_rays) without a GPU: the oracle's scene walk that the device is held to (tests/cpp/
ray_query_oracle.cpp) pinned to the reference's own records, and the ABI / Python surface of the new calls."""
import ctypes as C
import os
import struct

import numpy as np
import pytest

import kat_io
import ray_query_shim as shim
import raytracer_amd as ra
import ref_scenes

HERE = os.path.dirname(os.path.abspath(__file__))
RSQRT_TOLERANCE = 2.0 ** -11   # as tests/test_gpu_kat.py


def check_mesh_kat(hits, surfaces, occluded):
    """Query results on kat_io.mesh_fixture_scene() against mesh_kat.bin (the reference's MeshShape::Traverse / Traverse_Shadow /
    EvaluateIntersection on 4096 rays).  Scene::Traverse's one-object bypass rebuilds the local ray with BuildUnsafe (another rounding of invDir
    for box culling); measured: no ray of the fixture changes its record, so every record is held bit for bit.  The fixture's frame is the mesh's
    (MeshShape::EvaluateIntersection); the query returns the scene's (Scene::EvaluateIntersection, Scene.cpp:322-348): the normal through the
    object's (identity) transform -- the same values, where the +0 terms of x * row0 + y * row1 + z * row2 turn a -0 component into +0 -- and the
    tangent orthogonalised against it and normalised (:342), which is the fixture's tangent after that step within RSQRT_TOLERANCE."""
    kat_rays, exp, _ = shim.mesh_kat()
    hit = exp[:, 0] == 7
    assert hit.sum() > len(exp) // 4
    object_id = np.where(hit, 0, exp[:, 0]).astype(np.uint32)       # the fixture's object id 7 is scene object 0
    assert np.array_equal(hits[:, 1], object_id)
    assert np.array_equal(hits[:, 2], exp[:, 1])                     # triangle (0 on a miss)
    assert np.array_equal(hits[:, 0], exp[:, 2])                     # distance (tmax on a miss)
    assert np.array_equal(hits[:, 3], exp[:, 3]) and np.array_equal(hits[:, 4], exp[:, 4])   # u, v
    assert np.array_equal(occluded, exp[:, 5])                       # Traverse_Shadow
    n_ref, n_got = exp[hit][:, 10:13].view(np.float32), surfaces[hit][:, 3:6].view(np.float32)
    assert np.array_equal(n_ref, n_got)                              # as floats: -0 == +0
    assert np.array_equal(surfaces[hit][:, 9:11], exp[hit][:, 14:16])   # texCoord, bit for bit
    t_ref = exp[hit][:, 6:9].view(np.float32).astype(np.float64)
    n64 = n_ref.astype(np.float64)
    t_ref = t_ref - (t_ref * n64).sum(axis=1, keepdims=True) * n64
    t_ref /= np.linalg.norm(t_ref, axis=1, keepdims=True)
    t_got = surfaces[hit][:, 6:9].view(np.float32).astype(np.float64)
    assert np.all(np.abs(t_ref - t_got) <= RSQRT_TOLERANCE * np.maximum(np.abs(t_ref), 1e-3))
    return hit


def test_shim_reproduces_the_reference_mesh_records(built):
    scene, _, _ = kat_io.mesh_fixture_scene()
    kat_rays, _, _ = shim.mesh_kat()
    rays = shim.kat_query_rays(kat_rays)
    hits, surfaces, _ = shim.closest(scene.desc, rays)
    occluded, _ = shim.any_hit(scene.desc, rays)
    check_mesh_kat(hits, surfaces, occluded)


# share of the recorded vertices whose query record is identical to the reference's in every compared field, measured on this fixture set
EXACT_FLOORS = {"box_mesh": 0.84, "cornell": 0.70, "mesh_2k_all": 0.76, "mesh_single": 0.77}
ID_FLOORS = {"box_mesh": 1.0, "cornell": 0.9995, "mesh_2k_all": 1.0, "mesh_single": 1.0}


@pytest.mark.parametrize("name", sorted(EXACT_FLOORS))
def test_shim_agrees_with_the_reference_paths(built, name):
    """The vertices of the reference's own renderer (tests/golden/ref_paths, PathDebugData: ray, hit ids, distance, u, v, position, normal,
    uv) traced again as queries.  A recorded direction is already normalised and Ray() normalises it again, which can move its last bit; a
    secondary ray of the reference also carries the originDivDir of its un-offset origin, which a query's Ray() recomputes.  So the records are
    not all bit-identical: the ids must agree (floors below, measured), the values within tolerances, and the share of exactly identical
    records must not drop below what was measured (EXACT_FLOORS; box_mesh: flat-shaded boxes, the fewest rounding sites)."""
    raw = open(os.path.join(HERE, "golden", "ref_paths", name + ".bin"), "rb").read()
    magic, w, h, _, _, _, n, _ = struct.unpack("<8I", raw[:32])
    assert magic == 0x31565052
    v = np.frombuffer(raw, dtype=np.float32, offset=32).reshape(n, 28)
    u = v.view(np.uint32)
    scene, _ = ref_scenes.FIXTURES[name][0](w / h)
    hits, surfaces, _ = shim.closest(scene.desc, shim.pack(v[:, 0:3], v[:, 3:6], shim.INF))
    ids = (hits[:, 1] == u[:, 6]) & (hits[:, 2] == u[:, 7])
    hit = hits[:, 1] != ra.RT_INVALID_OBJECT
    assert ids.mean() >= ID_FLOORS[name]
    m = ids & hit
    dist = hits[:, 0].view(np.float32).astype(np.float64)
    assert np.all(np.abs(dist[m] - v[m, 8]) <= 5e-5 * np.maximum(v[m, 8], 1.0))
    assert np.all(np.abs(hits[m, 3:5].view(np.float32) - v[m, 9:11]) <= 5e-5)                                   # u, v
    sf = surfaces.view(np.float32)
    assert np.all(np.abs(sf[m, 0:3] - v[m, 11:14]) <= 2e-4 * np.maximum(np.abs(v[m, 11:14]), 1.0))               # position
    assert np.all(np.abs(sf[m, 3:6] - v[m, 14:17]) <= 1e-3)                                                      # normal
    assert np.all(np.abs(sf[m, 9:11] - v[m, 20:22]) <= 1e-4 * np.maximum(np.abs(v[m, 20:22]), 1.0))              # uv
    exact = ids & (hits[:, 0] == u[:, 8]) & (~hit | ((hits[:, 3] == u[:, 9]) & (hits[:, 4] == u[:, 10]) &
                                                     (surfaces[:, 0:3] == u[:, 11:14]).all(axis=1) & (sf[:, 3:6] == v[:, 14:17]).all(axis=1) &
                                                     (surfaces[:, 9:11] == u[:, 20:22]).all(axis=1)))
    assert exact.mean() >= EXACT_FLOORS[name], exact.mean()


def _header_offsets(struct_name):
    """sizeof / offsetof of an rtgpu.h record as the C compiler lays it out"""
    import subprocess
    import tempfile
    with tempfile.TemporaryDirectory() as d:
        fields = [f for f, _ in getattr(ra, struct_name)._fields_]
        body = "#include <stdio.h>\n#include <stddef.h>\n#include \"%s\"\nint main(){printf(\"%%zu\", sizeof(%s));%s printf(\"\\n\");return 0;}\n" % (
            os.path.join(shim.ROOT, "include", "rtgpu.h"), struct_name, "".join(' printf(" %%zu", offsetof(%s, %s));' % (struct_name, f) for f in fields))
        src, exe = os.path.join(d, "o.c"), os.path.join(d, "o")
        open(src, "w").write(body)
        subprocess.check_call(["gcc", src, "-o", exe])
        return [int(x) for x in subprocess.check_output([exe]).split()]


@pytest.mark.parametrize("struct_name", ["RtQueryRay", "RtQueryHit", "RtQuerySurface"])
def test_ctypes_records_match_the_header(struct_name):
    t = getattr(ra, struct_name)
    assert _header_offsets(struct_name) == [C.sizeof(t)] + [getattr(t, f).offset for f, _ in t._fields_]
    assert C.sizeof(t) % 16 == 0


def test_query_entry_points_are_exported(built):
    lib = ra.rtgpu_lib()
    for name in ("rtgpu_trace_rays", "rtgpu_trace_rays_async"):
        assert hasattr(lib, name)


def test_trace_rays_rejects_bad_input_before_the_device(built):
    scene, camera = ref_scenes.FIXTURES["box_mesh"][0](1.0)
    vp = ra.Viewport(8, 8)
    o = np.zeros((4, 3), dtype=np.float32)
    d = np.ones((4, 3), dtype=np.float32)
    for bad_o, bad_d in ((o[:, :2], d[:, :2]), (o.astype(np.float64), d), (o, d[:3]), (o.reshape(-1), d.reshape(-1)), (o.tolist(), d)):
        with pytest.raises(ValueError):
            vp.trace_rays(bad_o, bad_d)
        with pytest.raises(ValueError):
            vp.occluded(bad_o, bad_d)
    with pytest.raises(ValueError):
        vp.trace_rays(o, d, max_distance=np.ones(3, dtype=np.float32))
    with pytest.raises(RuntimeError):   # no renderer
        vp.trace_rays(o, d)


def test_query_without_a_device_raises(built):
    """No CPU fallback: without a device, set_renderer followed by a query raises RuntimeError (with one, the same lines answer)."""
    try:
        n = C.c_int(0)
        have_device = C.CDLL("libamdhip64.so").hipGetDeviceCount(C.byref(n)) == 0 and n.value > 0
    except OSError:
        have_device = False
    scene, _ = ref_scenes.FIXTURES["box_mesh"][0](1.0)
    vp = ra.Viewport(8, 8)

    def query():
        vp.set_renderer(scene)
        return vp.trace_rays(np.zeros((2, 3), dtype=np.float32), np.ones((2, 3), dtype=np.float32))
    if have_device:
        assert query().distance.shape == (2,)
    else:
        with pytest.raises(RuntimeError):
            query()
