"""The oracle's scene walk behind the ray queries of include/rtgpu.h (tests/cpp/ray_query_oracle.cpp), the random ray sets the query tests use,
and the reference's mesh_kat.bin records.  Records travel as raw uint32 words: (N, 8) RtQueryRay, (N, 8) RtQueryHit, (N, 12) RtQuerySurface."""
import ctypes as C
import os
import subprocess

import numpy as np

import raytracer_amd as ra

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "ray_query_oracle.cpp")
LIB = os.path.join(ROOT, "tests", "cpp", "_build", "libray_query_oracle.so")
ORACLE_FLAGS = ["-O2", "-std=c++17", "-fPIC", "-ffp-contract=off", "-mavx2", "-mfma"]   # oracle/Makefile's CXXFLAGS (warnings aside)
INF = np.float32(np.inf)

_lib = None


def lib():
    """Builds the shim (with the oracle Makefile's flags) into tests/cpp/_build once per process."""
    global _lib
    if _lib is None:
        deps = [SRC, os.path.join(ROOT, "oracle", "rto_core.h"), os.path.join(ROOT, "oracle", "rto_math.h"), os.path.join(ROOT, "include", "rtgpu.h")]
        if not os.path.exists(LIB) or any(os.path.getmtime(d) > os.path.getmtime(LIB) for d in deps):
            os.makedirs(os.path.dirname(LIB), exist_ok=True)
            subprocess.check_call([os.environ.get("CXX", "g++")] + ORACLE_FLAGS + ["-shared", "-o", LIB + ".tmp", SRC])
            os.replace(LIB + ".tmp", LIB)
        _lib = C.CDLL(LIB)
    return _lib


def pack(origins, directions, max_distance):
    rays = np.zeros((len(origins), 8), dtype=np.float32)
    rays[:, 0:3], rays[:, 3], rays[:, 4:7] = origins, max_distance, directions
    return rays


def closest(desc, rays, surfaces=True):
    """(hits (N, 8) uint32, surfaces (N, 12) uint32 or None, counters (16,) uint64)"""
    n = len(rays)
    hits = np.zeros((n, 8), dtype=np.uint32)
    surf = np.zeros((n, 12), dtype=np.uint32) if surfaces else None
    cnt = np.zeros(16, dtype=np.uint64)
    lib().rqo_trace_closest(desc, np.ascontiguousarray(rays).ctypes.data_as(C.c_void_p), C.c_uint32(n), hits.ctypes.data_as(C.c_void_p),
                            surf.ctypes.data_as(C.c_void_p) if surfaces else None, cnt.ctypes.data_as(C.c_void_p))
    return hits, surf, cnt


def any_hit(desc, rays):
    """(occluded (N,) uint32, counters (16,) uint64)"""
    n = len(rays)
    occ = np.zeros(n, dtype=np.uint32)
    cnt = np.zeros(16, dtype=np.uint64)
    lib().rqo_trace_any(desc, np.ascontiguousarray(rays).ctypes.data_as(C.c_void_p), C.c_uint32(n), occ.ctypes.data_as(C.c_void_p), cnt.ctypes.data_as(C.c_void_p))
    return occ, cnt


def scene_bounds(scene):
    """World-space box of the scene: the top-level root, or the single object's mesh root taken through its transform."""
    d = scene.desc.contents
    if d.numTopNodes:
        n = d.topNodes[0]
        return np.array(n.min[:], dtype=np.float64), np.array(n.max[:], dtype=np.float64)
    obj = d.objects[0]
    mesh = d.meshes[obj.meshIndex]
    n = d.meshNodes[mesh.firstNode]
    lo, hi = np.array(n.min[:]), np.array(n.max[:])
    m = np.array(obj.transform[:], dtype=np.float64).reshape(4, 4)
    corners = np.array([[x, y, z, 1.0] for x in (lo[0], hi[0]) for y in (lo[1], hi[1]) for z in (lo[2], hi[2])]) @ m
    return corners[:, :3].min(axis=0), corners[:, :3].max(axis=0)


def random_rays(scene, n, seed):
    """n rays over the scene: origins inside and around its bounds, directions with exactly-zero components in a quarter of them (the 0 * inf
    slab cases), maxDistance +inf for a third, finite for a third, and for the last third just below the distance of the ray's own closest hit
    (the oracle's, with +inf; +inf where the ray misses)."""
    rng = np.random.RandomState(seed)
    lo, hi = scene_bounds(scene)
    ext = hi - lo
    origins = (lo - 0.25 * ext + rng.rand(n, 3) * 1.5 * ext).astype(np.float32)
    dirs = rng.normal(size=(n, 3)).astype(np.float32)
    zero = rng.rand(n) < 0.25
    axes = rng.randint(0, 3, size=n)
    dirs[zero, axes[zero]] = 0.0
    two = zero & (rng.rand(n) < 0.3)
    dirs[two, (axes[two] + 1) % 3] = 0.0
    dirs[np.all(dirs == 0.0, axis=1), 2] = 1.0
    maxd = np.full(n, INF, dtype=np.float32)
    third = n // 3
    maxd[third:2 * third] = (0.05 + rng.rand(third) * np.linalg.norm(ext)).astype(np.float32)
    rays = pack(origins, dirs, maxd)
    last = np.arange(2 * third, n)
    probe = rays[last].copy()
    probe[:, 3] = INF
    hits, _, _ = closest(scene.desc, probe, surfaces=False)
    d = hits[:, 0].view(np.float32)
    hit = hits[:, 1] != ra.RT_INVALID_OBJECT
    rays[last[hit], 3] = np.nextafter(d[hit], np.float32(0.0))
    return rays


def mesh_kat():
    """The reference's MeshShape::Traverse / Traverse_Shadow / EvaluateIntersection records of tests/golden/mesh_kat.bin: (rays (N, 7) float32
    {origin, direction, tmax}, expected (N, 19) uint32 {objectId (7 on a hit), triangle, distance, u, v, anyHit, tangent[4], normal[4], texCoord[4],
    material (local)}, local -> global material map)."""
    raw = np.fromfile(os.path.join(ROOT, "tests", "golden", "mesh_kat.bin"), dtype=np.uint32)
    num_nodes, num_tris = int(raw[0]), int(raw[1])
    off = 2 + 8 * num_nodes
    ref_tris = raw[off:off + 13 * num_tris].reshape(num_tris, 13)
    off += 13 * num_tris
    num_rays = int(raw[off])
    off += 1
    rec = raw[off:off + 26 * num_rays].reshape(num_rays, 26)
    return rec[:, :7].copy().view(np.float32), rec[:, 7:].copy(), ref_tris


def kat_query_rays(kat_rays):
    return pack(kat_rays[:, 0:3], kat_rays[:, 3:6], kat_rays[:, 6])
