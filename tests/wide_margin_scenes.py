"""Geometry and rays placed on purpose where the 4-wide walks' exactness margins are thin (rt_wide_grid.inl, rt_wide_walk.h), and a NumPy model of those
margins.  Pure NumPy plus raytracer_amd.Scene; everything is seeded, nothing reads files.

The margins:  the spare grid step (wideQuantiseBox; wideGridHolds decides whether a mesh gets a 4-wide tree at all), the fold trust test
(RT_WIDE_FOLD_TEST: m * 2^-21 < step * |invDir| per axis, m = |originDivDir| + bound * |invDir|; since both sides carry |invDir| this is
|origin| + bound < 2^21 * step ~ 32 extents of the mesh's box on that axis), the runner-up tolerance (RT_WIDE_FOLD_TOL) and the any-hit leaf gate against
the fixed ray length.  Mesh families: offset, layers, flat / sliver_box, two_level.  Ray families: aimed, tiny_components, grazing."""
import ctypes as C

import numpy as np

import ray_query_shim as shim
import raytracer_amd as ra

F32 = np.float32
FLT_MAX = float(np.finfo(np.float32).max)
NUM_RAYS = 16384
QUANT_GRID = F32(65535.0)
FOLD = F32(2.0 ** -21)
BAND = 0.01   # of the model: NumPy's and the device's normalisation of a direction differ by ulps, a ray inside the band is "borderline"


# ---- the model ----------------------------------------------------------------------------------------------------------------------------
def grid_over(lo, hi):
    """wideGridOver + wideGridHolds (rt_scene_prepare.h) in float32 / double as there: (base, step, bound, holds)."""
    lo, hi = np.asarray(lo, dtype=F32), np.asarray(hi, dtype=F32)
    largest = F32((hi - lo).max())
    step = np.maximum(hi - lo, F32(1e-6) * max(largest, F32(1e-30))) / (QUANT_GRID - F32(8.0))
    base = lo - F32(4.0) * step
    bound = np.maximum(np.abs(lo), np.abs(hi)) + F32(8.0) * step
    b, s = base.astype(np.float64), step.astype(np.float64)
    holds = bool(np.all(step > 0) and np.all(np.isfinite(step)) and np.all(b <= lo.astype(np.float64) - 0.5 * s) and np.all(b + 65535.0 * s >= hi.astype(np.float64) + 0.5 * s))
    return base.astype(F32), step.astype(F32), bound.astype(F32), holds


def mesh_root_box(scene, mesh_index=0):
    d = scene.desc.contents
    n = d.meshNodes[d.meshes[mesh_index].firstNode]
    return np.array(n.min[:], dtype=F32), np.array(n.max[:], dtype=F32)


def scene_grid(scene, mesh_index=0):
    return grid_over(*mesh_root_box(scene, mesh_index))


def trust_model(rays, base, step, bound):
    """RT_WIDE_FOLD_TEST for rays of RtQueryRay words against a mesh entered under the identity transform: (clearly trusted, clearly untrusted,
    borderline) masks.  The float32 terms are the device's (makeRay normalises, makeRayUnsafe3 divides); "clearly" means the comparison still goes
    the same way with both sides moved 1 % against it, and a quotient that overflows does so by 1 %."""
    o, d = rays[:, 0:3].astype(F32), rays[:, 4:7].astype(F32)
    base, step, bound = (np.asarray(a, dtype=F32) for a in (base, step, bound))
    with np.errstate(all="ignore"):
        length = np.sqrt((d * d).sum(axis=1, dtype=F32), dtype=F32)
        direction = d * (F32(1.0) / length)[:, None]
        inv = F32(1.0) / direction
        odd = o * inv
        m = np.abs(odd) + bound * np.abs(inv)
        lhs, rhs = (m * FOLD).astype(np.float64), (step * np.abs(inv)).astype(np.float64)
        # finiteness, judged in double on the same inputs
        inv64 = np.abs(1.0 / direction.astype(np.float64))
        big = np.maximum(inv64, np.abs(o.astype(np.float64)) * inv64 + bound.astype(np.float64) * inv64)
        big = np.where(np.isnan(big), np.inf, big)
        surely_finite = (big * (1.0 + BAND) < FLT_MAX).all(axis=1)
        surely_not = (np.maximum(inv64, np.abs(o.astype(np.float64)) * inv64) * (1.0 - BAND) > FLT_MAX).any(axis=1) | (direction == 0).any(axis=1)
        trusted = surely_finite & (lhs * (1.0 + BAND) < rhs * (1.0 - BAND)).all(axis=1)
        untrusted = surely_not | (surely_finite & (lhs * (1.0 - BAND) >= rhs * (1.0 + BAND)).any(axis=1))
    return trusted, untrusted, ~(trusted | untrusted)


def model_class(trusted, untrusted, i):
    return "trusted" if trusted[i] else ("untrusted" if untrusted[i] else "borderline")


# ---- meshes -------------------------------------------------------------------------------------------------------------------------------
def sheet(n=32, seed=1, amp=0.15, jitter=0.02, offset=(0.0, 0.0, 0.0), scale=(1.0, 1.0, 1.0)):
    """n x n quads over [-0.5, 0.5]^2 in x, z (extent 1) with a sine relief and seeded jitter in y; vertex COORDINATES displaced by `offset`."""
    rng = np.random.RandomState(seed)
    g = np.linspace(-0.5, 0.5, n + 1)
    x, z = np.meshgrid(g, g)
    y = amp * np.sin(7 * x) * np.cos(5 * z) + jitter * rng.standard_normal(x.shape)
    pos = (np.stack([x, y, z], -1).reshape(-1, 3) * np.asarray(scale, dtype=np.float64) + np.asarray(offset, dtype=np.float64)).astype(F32)
    i = np.arange(n * n)
    r, c = i // n, i % n
    a = r * (n + 1) + c
    idx = np.concatenate([np.stack([a, a + n + 2, a + 1], -1), np.stack([a, a + n + 1, a + n + 2], -1)]).astype(np.uint32)   # wound so that the faces look up (+y)
    return pos, idx


# displacement in extents, chosen by the model over aimed(1.5) rays (tests/test_wide_margins_cpu.py asserts the shares): per direction one clearly
# trusted, borderline ones, one with no ray trusted and one where wideGridHolds fails
OFFSETS = {
    "diag": {"trusted": 4.0, "borderline": (5.25, 5.5, 5.75), "untrusted": 8.0, "no_grid": 4096.0},
    "x": {"trusted": 12.0, "borderline": (15.25, 15.5, 15.75), "untrusted": 24.0, "no_grid": 4096.0},
}


def offset_mesh(k, axis):
    return sheet(offset=(k, k, k) if axis == "diag" else (k, 0.0, 0.0))


LAYER_ULPS = (0, 1, 2, 8, 16, 32, 64, 256, 4096, 65536)
LAYER_SHEETS, LAYER_QUADS = 8, 6
OBLIQUE_NORMAL = np.array([0.3, 0.9, 0.316])


def layers_frame(oblique):
    """(unit normal, in-plane unit vector `side`) of the stack"""
    nrm = OBLIQUE_NORMAL / np.linalg.norm(OBLIQUE_NORMAL) if oblique else np.array([0.0, 1.0, 0.0])
    side = np.cross(nrm, [1.0, 0.0, 0.0])
    return nrm, side / np.linalg.norm(side)


LAYER_STAGGER = 0.08   # frames: half a quad per copy


def layers_mesh(k_ulps, oblique, stagger=0.0):
    """Eight copies of a flat 6 x 6-quad sheet, each moved from the previous one by k_ulps units in the last place of every coordinate along the
    sheet's normal (y, or OBLIQUE_NORMAL: then hit distances differ in all three slab terms).  Vertex v of copy s is vertex s * 49 + v.
    `stagger`: copy s also slides s * stagger along `side` within its plane, so that every copy shows a strip of itself beside the copies above, which
    overhang it k_ulps, 2 k_ulps, ... higher: a next-event ray that leaves such a strip towards +side passes under them."""
    base, bidx = sheet(LAYER_QUADS, 5, amp=0.0, jitter=0.0)
    base = base.astype(np.float64)
    base[:, 1] = 0.25
    nrm = np.array([0.0, 1.0, 0.0])
    if oblique:
        nrm = OBLIQUE_NORMAL / np.linalg.norm(OBLIQUE_NORMAL)
        a = np.cross([0.0, 1.0, 0.0], nrm)
        sn = np.linalg.norm(a)
        a /= sn
        K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
        base = base @ (np.eye(3) + sn * K + (1.0 - nrm[1]) * K @ K).T
    along = (np.sign(nrm) * (np.abs(nrm) > 0.1)).astype(F32)
    side = layers_frame(oblique)[1]
    P, I = [], []
    for s in range(LAYER_SHEETS):
        cur = (base + s * stagger * side).astype(F32)
        for _ in range(s):
            cur = (cur + np.spacing(np.abs(cur)) * F32(k_ulps) * along).astype(F32)
        P.append(cur)
        I.append(bidx + s * len(base))
    return np.concatenate(P), np.concatenate(I).astype(np.uint32)


def flat_mesh(y):
    pos, idx = sheet(amp=0.0, jitter=0.0)
    pos[:, 1] = F32(y)
    return pos, idx


def sliver_box_mesh():
    """the bumpy sheet in a box of extents 1e4 : 1e-3 : 1 (x : y : z)"""
    pos, idx = sheet()
    pos = pos.astype(np.float64)
    y = pos[:, 1]
    pos[:, 1] = (y - y.min()) / (y.max() - y.min()) * 1e-3
    pos[:, 0] *= 1e4
    return pos.astype(F32), idx


def vertex_frames(pos, idx):
    """(normals, tangents) per vertex for shading: area-weighted face normals (in double, from the float32 positions) and a unit vector across them"""
    p = pos.astype(np.float64)
    face = np.cross(p[idx[:, 1]] - p[idx[:, 0]], p[idx[:, 2]] - p[idx[:, 0]])
    face /= np.maximum(np.linalg.norm(face, axis=1, keepdims=True), 1e-300)   # (unit: a sheet displaced by thousands of extents still has triangles of any area)
    n = np.zeros_like(p)
    for k in range(3):
        np.add.at(n, idx[:, k], face)
    length = np.linalg.norm(n, axis=1, keepdims=True)
    n = np.where(length > 0.0, n / np.maximum(length, 1e-300), [0.0, 1.0, 0.0])
    t = np.cross(n, np.where(np.abs(n[:, :1]) < 0.9, [1.0, 0.0, 0.0], [0.0, 0.0, 1.0]))
    t /= np.linalg.norm(t, axis=1, keepdims=True)
    return n.astype(F32), t.astype(F32)


def add_mesh(s, pos, idx, material, transform=None):
    n, t = vertex_frames(pos, idx)
    s.add_mesh(pos, idx, n, t, default_material=material, transform=transform)


def single_mesh_scene(pos, idx, lights=None):
    s = ra.Scene()
    add_mesh(s, pos, idx, s.add_material("diffuse", (0.7, 0.6, 0.5)))
    s.add_background_light((1.0, 1.5, 2.0))
    if lights:
        lights(s)
    s.build()
    return s


def two_level_scene(pos, idx, lights=None):
    """The mesh as two objects of a two-level scene -- the second an instance -- under rotations with translations of 0 and 1e3 extents, and one
    analytic sphere (radius 5e3 extents) 1e4 extents away: a top-level grid that is coarse against the objects, mesh levels entered through invTransform at large magnitude."""
    lo, hi = pos.min(0).astype(np.float64), pos.max(0).astype(np.float64)
    ext = float(np.linalg.norm(hi - lo))
    s = ra.Scene()
    m = s.add_material("diffuse", (0.7, 0.6, 0.5))
    add_mesh(s, pos, idx, m, ra.transform_from_euler((0.0, 0.0, 0.0), (20.0, 35.0, 10.0)))
    s.add_instance(0, ra.transform_from_euler((1e3 * ext, 0.0, 0.0), (-15.0, 50.0, 25.0)), m)
    s.add_sphere(5e3 * ext, ra.transform_from_euler((0.0, 1e4 * ext, 0.0)), s.add_material("diffuse", (0.3, 0.8, 0.4)))   # (large enough for bounce rays to find it)
    s.add_background_light((1.0, 1.5, 2.0))
    if lights:
        lights(s)
    s.build()
    return s


def mesh_families():
    """{name: (positions, indices)} of every single-mesh family member, in a fixed order."""
    out = {"centred": offset_mesh(0.0, "x")}
    for axis, ks in OFFSETS.items():
        for k in (ks["trusted"],) + tuple(ks["borderline"]) + (ks["untrusted"], ks["no_grid"]):
            out["offset_%s_%g" % (axis, k)] = offset_mesh(k, axis)
    for oblique in (False, True):
        for k in LAYER_ULPS:
            out["layers_%s_%d" % ("oblique" if oblique else "y", k)] = layers_mesh(k, oblique)
    out["flat_0"] = flat_mesh(0.0)
    out["flat_0.25"] = flat_mesh(0.25)
    out["sliver_box"] = sliver_box_mesh()
    return out


# ---- rays ---------------------------------------------------------------------------------------------------------------------------------
def _unit(rng, n):
    d = rng.standard_normal((n, 3))
    return d / np.linalg.norm(d, axis=1, keepdims=True)


def with_max_distance(scene, origins, dirs, seed):
    """RtQueryRay words; maxDistance +inf for a third, finite for a third, and for a third just below the oracle's own hit distance (as shim.random_rays)."""
    n = len(origins)
    rng = np.random.RandomState(seed)
    rays = shim.pack(np.asarray(origins, dtype=F32), np.asarray(dirs, dtype=F32), np.full(n, np.inf, dtype=F32))
    hits, _, _ = shim.closest(scene.desc, rays, surfaces=False)
    dist = hits[:, 0].view(F32)
    hit = hits[:, 1] != ra.RT_INVALID_OBJECT
    third = n // 3
    scale = float(np.median(dist[hit])) if hit.any() else 1.0
    rays[third:2 * third, 3] = (scale * (0.05 + 1.5 * rng.rand(third))).astype(F32)
    last = np.arange(2 * third, n)
    last = last[hit[last]]
    rays[last, 3] = np.nextafter(dist[last], F32(0.0))
    return rays


def _targets(pos, rng, n):
    """jittered mesh vertices -- per axis by 1 % of the box's extent there (of the largest extent on an axis without any), a quarter of them by 30 %, so
    that many of those rays miss -- and the length of the box's diagonal, the "extent" ray distances are counted in"""
    size = pos.max(0).astype(np.float64) - pos.min(0).astype(np.float64)
    sigma = np.where(rng.rand(n, 1) < 0.25, 0.3, 0.01) * np.where(size > 0.0, size, size.max())
    return pos[rng.randint(0, len(pos), n)].astype(np.float64) + sigma * rng.standard_normal((n, 3)), np.linalg.norm(size)


AIMED_DISTANCES = (1.5, 10.0, 30.0, 80.0, 1e3, 1e5)
# the meshes that meet every start distance: the centred sheet (the graded shares of the trust test), the benign end of either offset direction, and the
# degenerate grids
SWEPT_MESHES = ("centred",) + tuple("offset_%s_%g" % (axis, OFFSETS[axis]["trusted"]) for axis in sorted(OFFSETS)) + ("flat_0", "sliver_box")


def families_of(mesh):
    """the ray families a mesh family member meets.  The sliver box stops at 80 extents: from 1e3 of them (1e7 units) a float32 origin moves in steps of 1,
    a thousand times the box's thickness, and "aimed" rays no longer are (1 % of them hit)."""
    far = 1e3 if mesh == "sliver_box" else np.inf
    return ("aimed_1.5", "tiny_components", "grazing") + (tuple("aimed_%g" % d for d in AIMED_DISTANCES[1:] if d < far) if mesh in SWEPT_MESHES else ())


def aimed(scene, pos, distance, seed=2, n=NUM_RAYS):
    """targets: jittered mesh vertices; origins `distance` extents (x 0.2 .. 1) back along a random direction"""
    rng = np.random.RandomState(seed)
    tgt, ext = _targets(pos, rng, n)
    d = _unit(rng, n)
    o = tgt - d * distance * ext * rng.uniform(0.2, 1.0, (n, 1))
    return with_max_distance(scene, o, d, seed + 100)


TINY = (1e-8, -1e-8, 1e-20, -1e-20, 1e-37, -1e-37, 1e-39, 1e-44)


def tiny_components(scene, pos, seed=3, n=NUM_RAYS):
    """aimed at 1.5 extents with one direction component replaced by a tiny value (the last two are float32 denormals): invDir is huge, or infinite
    without the component being zero -- then rayIsNaNFree must send the ray to the binary walk.  The origin is taken back from the target along the
    replaced direction, so the rays still meet the mesh."""
    rng = np.random.RandomState(seed)
    tgt, ext = _targets(pos, rng, n)
    d = _unit(rng, n)
    i = np.arange(n)
    d[i, i % 3] = np.asarray(TINY)[(i // 3) % len(TINY)]
    d32 = d.astype(F32)
    dn = d32.astype(np.float64) / np.linalg.norm(d32.astype(np.float64), axis=1, keepdims=True)
    o = tgt - dn * 1.5 * ext * rng.uniform(0.2, 1.0, (n, 1))
    return with_max_distance(scene, o, d32, seed + 100)


def leaf_corners(scene, mesh_index=0):
    d = scene.desc.contents
    mesh = d.meshes[mesh_index]
    words = node_words(scene, mesh_index)
    leaves = words[(words[:, 7] & 0x3FFFFFFF) != 0]
    lo, hi = leaves[:, 0:3].view(F32), leaves[:, 4:7].view(F32)
    pick = np.array([[x, y, z] for x in (0, 1) for y in (0, 1) for z in (0, 1)], dtype=bool)
    return np.concatenate([np.where(p, hi, lo) for p in pick])


def node_words(scene, mesh_index=0):
    """the mesh's RtNode records as (numNodes, 8) uint32 words: min.xyz, childIndex, max.xyz, leaves"""
    d = scene.desc.contents
    mesh = d.meshes[mesh_index]
    return np.ctypeslib.as_array(C.cast(C.addressof(d.meshNodes[mesh.firstNode]), C.POINTER(C.c_uint32 * 8 * mesh.numNodes)).contents)


def grazing(scene, pos, idx, seed=4, n=NUM_RAYS):
    """Five equal parts.  0: rays through exact float32 vertices (direction = vertex - origin in float32, not normalised); 1: through the float32
    midpoints of triangle edges (shared by two triangles inside the sheet); 2: rays that lie in the plane y = a vertex's y (direction y exactly 0:
    the plane of the sheet for `flat`); 3: rays whose origin is a hit point of the oracle (t = 0 on a triangle); 4: rays whose origin is a corner of
    a leaf box of the mesh's tree."""
    rng = np.random.RandomState(seed)
    part = n // 5
    ext = np.linalg.norm(pos.max(0).astype(np.float64) - pos.min(0).astype(np.float64))
    O, D = [], []
    # 0, 1: through vertices and edge midpoints
    tri = idx[rng.randint(0, len(idx), part)]
    e = rng.randint(0, 3, part)
    a, b = pos[tri[np.arange(part), e]], pos[tri[np.arange(part), (e + 1) % 3]]
    for tgt in (pos[rng.randint(0, len(pos), part)], ((a + b) * F32(0.5)).astype(F32)):
        o = (tgt.astype(np.float64) - _unit(rng, part) * ext * rng.uniform(0.3, 1.5, (part, 1))).astype(F32)
        O.append(o)
        D.append((tgt.astype(np.float64) - o.astype(np.float64)).astype(F32))
    # 2: in the plane of a vertex's y
    v = pos[rng.randint(0, len(pos), part)].astype(np.float64)
    d = _unit(rng, part)
    d[:, 1] = 0.0
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    o = (v - d * ext * rng.uniform(0.3, 1.5, (part, 1))).astype(F32)
    o[:, 1] = v[:, 1].astype(F32)
    O.append(o)
    D.append(d.astype(F32))
    # 3: from the oracle's hit points
    probe = aimed(scene, pos, 1.5, seed + 50, 4 * part)
    probe[:, 3] = np.inf
    hits, surf, _ = shim.closest(scene.desc, probe, surfaces=True)
    at = surf[hits[:, 1] != ra.RT_INVALID_OBJECT][:, 0:3].view(F32)
    at = at[np.arange(part) % max(len(at), 1)] if len(at) else pos[rng.randint(0, len(pos), part)]
    O.append(at)
    D.append(_unit(rng, part).astype(F32))
    # 4: from leaf-box corners, half of them towards a vertex
    corners = leaf_corners(scene)
    rest = n - 4 * part
    o = corners[rng.randint(0, len(corners), rest)]
    d = _unit(rng, rest)
    towards = pos[rng.randint(0, len(pos), rest)].astype(np.float64) - o.astype(np.float64)
    use = (rng.rand(rest) < 0.5) & (np.linalg.norm(towards, axis=1) > 1e-3 * ext)
    d[use] = towards[use]
    O.append(o)
    D.append(d.astype(F32))
    return with_max_distance(scene, np.concatenate(O), np.concatenate(D), seed + 100)


def ray_families(scene, pos, idx, which):
    """the rays of family `which`: "aimed_<distance>", "tiny_components" or "grazing" """
    if which.startswith("aimed_"):
        return aimed(scene, pos, float(which[6:]))
    return tiny_components(scene, pos) if which == "tiny_components" else grazing(scene, pos, idx)


def hit_sheet(scene, hits):
    """for layers_mesh: the copy (0 .. 7) each hit's triangle belongs to, -1 for a miss"""
    d = scene.desc.contents
    words = np.ctypeslib.as_array(C.cast(d.vertexIndices, C.POINTER(C.c_uint32 * 4 * d.numTriangles)).contents)
    hit = hits[:, 1] != ra.RT_INVALID_OBJECT
    out = np.full(len(hits), -1, dtype=np.int64)
    out[hit] = words[hits[hit, 2], 0] // ((LAYER_QUADS + 1) ** 2)
    return out


# ---- frames: the 4-wide any-hit walk (queries never reach it) --------------------------------------------------------------------------------
def look_at(eye, target):
    """Euler angles (degrees) whose local +z axis points from eye to target.  Quaternion::FromEulerAngles turns +z into
    (sin yaw cos pitch, -sin pitch, cos yaw cos pitch)."""
    d = np.asarray(target, dtype=np.float64) - np.asarray(eye, dtype=np.float64)
    d /= np.linalg.norm(d)
    angles = (float(-np.degrees(np.arcsin(np.clip(d[1], -1.0, 1.0)))), float(np.degrees(np.arctan2(d[0], d[2]))), 0.0)
    m = np.array(ra.transform_from_euler((0.0, 0.0, 0.0), angles)[:]).reshape(4, 4)
    assert float(m[2, :3] @ d) > 0.9999, (angles, m[2, :3], d)
    return angles


def ulps(x, k):
    """the float32 k units in the last place above (k > 0) or below x"""
    x = F32(x)
    for _ in range(abs(k)):
        x = np.nextafter(x, F32(np.inf if k > 0 else -np.inf))
    return float(x)


def _sheet_lights(centre, normal, ext, point=True, low=False):
    """a point light above the sheet (a scene object of its own: the scene is then walked on two levels) and a one-degree directional light.
    `low`: the point light stands 16 degrees above the sheet's plane on its +side (for the staggered layers: its rays pass under the overhanging copies, and
    the 1e-4 shadow offset lifts their origin 2.8e-5 above the sheet they leave)."""
    def lights(s):
        n = np.asarray(normal, dtype=np.float64) / np.linalg.norm(normal)
        side = np.cross(n, [1.0, 0.0, 0.0])
        side /= np.linalg.norm(side)
        at = np.asarray(centre, dtype=np.float64) + ext * ((0.004 * n + 2.0 * side) if low else (0.8 * n + 0.15 * side))
        if point:
            s.add_point_light((6.0, 5.5, 5.0), ra.transform_from_euler(tuple(at.astype(F32)), (0.0, 0.0, 0.0)))
        s.add_directional_light((3.0, 3.0, 2.5), F32(1.0) / F32(180.0) * F32(3.14159265359), ra.transform_from_euler((0.0, 0.0, 0.0), look_at(n + 0.3 * side, (0.0, 0.0, 0.0))))
    return lights


def _sheet_camera(centre, normal, ext, aspect):
    """2 extents from the sheet, looking at its centre"""
    n = np.asarray(normal, dtype=np.float64) / np.linalg.norm(normal)
    side = np.cross(n, [1.0, 0.0, 0.0])
    side /= np.linalg.norm(side)
    eye = np.asarray(centre, dtype=np.float64) + 2.0 * ext * (0.6 * n - 0.8 * side)
    return ra.Camera(tuple(float(v) for v in eye.astype(F32)), look_at(eye, centre), aspect, 40.0)


ROOM_HEIGHT = 1.0


def room_mesh(tiny_copy_about=None):
    """One mesh: the bumpy sheet (16 x 16 quads) as a floor around y = 0 and a flat ceiling sheet three times as wide at y = ROOM_HEIGHT; with
    `tiny_copy_about` = L, no ceiling but a small image of the floor under L: vertex p goes to L - (1e-3 |L - p| - 1e-4) u, u the unit vector from p to L.
    A next-event ray from a floor point p to a point light at L starts 1e-4 along u and is 0.999 |L - p| long (PathTracerMIS::SampleLight), so it meets
    the image of p where it ends.  Inside an image triangle the surface leaves that locus by ~1e-4 x (the triangle's angular size)^2 / 8 ~ 5e-8: the fixed
    ray length lies within an ulp of a hit, on either side -- the case the leaf gate's entry-distance test and include/rtgpu.h's caveat are about."""
    floor, fidx = sheet(16, 7)
    if tiny_copy_about is None:
        other, oidx = sheet(8, 8, amp=0.0, jitter=0.0, scale=(3.0, 1.0, 3.0), offset=(0.0, ROOM_HEIGHT, 0.0))
    else:
        to_light = np.asarray(tiny_copy_about, dtype=np.float64) - floor.astype(np.float64)
        dist = np.linalg.norm(to_light, axis=1, keepdims=True)
        other, oidx = (np.asarray(tiny_copy_about, dtype=np.float64) - (1e-3 * dist - 1e-4) * to_light / dist).astype(F32), fidx
    return np.concatenate([floor, other]), np.concatenate([fidx, oidx + len(floor)]).astype(np.uint32)


def _room_camera(aspect):
    eye = (0.0, 0.55, -1.1)
    return ra.Camera(eye, look_at(eye, (0.0, 0.0, 0.0)), aspect, 45.0)


LAYER_FRAME_ULPS = (0, 1, 16, 256, 4096)
FRAME_CASES = (["offset_%s" % r for r in ("trusted", "borderline", "untrusted", "no_grid")] + ["sun_offset_%s" % r for r in ("trusted", "borderline", "untrusted", "no_grid")] +
               ["layers_oblique_%d" % k for k in LAYER_FRAME_ULPS] +
               ["rect_below_%d" % k for k in (0, 1, 4, 64)] + ["rect_above_%d" % k for k in (1, 4, 64)] + ["rect_far_above_no_background"] +
               ["point_on_vertex", "point_1ulp_behind_ceiling", "point_homothetic"] + ["two_level_offset_borderline", "two_level_layers_oblique_1"])
# the one frame in which no light reaches anything: the rect light lies 5 % of the room's height above a ceiling three times as wide as the floor, so every
# next-event ray -- 0.1 % shorter than the way to the light -- meets the ceiling first; the scene has no background light.  Every other case lets light through:
# a light k <= 64 ulps (< 1e-5 of the room's height) beyond a sheet is nearer to it than the 0.1 % a next-event ray stops short of the light.
ALL_OCCLUDED = ("rect_far_above_no_background",)


def frame_case(name, aspect):
    """(scene, camera, serving walk expected with the counters off).  A light with a place in the scene (point, area) is a scene object: such a scene has a
    top level and k_trace_wide2 walks it; "sun_" cases keep the directional and the background light only, so that the mesh is the scene's one object and
    k_trace_wide / k_tail walk it -- either kernel's any-hit walk meets every offset regime."""
    if "offset_" in name:
        regime = name.split("offset_")[-1]
        k = OFFSETS["diag"][regime][1] if regime == "borderline" else OFFSETS["diag"][regime]
        pos, idx = offset_mesh(k, "diag")
        centre, normal = (k, k, k), (0.0, 1.0, 0.0)
    elif "layers_oblique" in name:
        pos, idx = layers_mesh(int(name.split("_")[-1]), True, stagger=0.0 if name.startswith("two_level") else LAYER_STAGGER)
        centre, normal = 0.5 * (pos.min(0).astype(np.float64) + pos.max(0)), OBLIQUE_NORMAL
    if name.startswith("two_level"):
        lo, hi = pos.min(0).astype(np.float64), pos.max(0).astype(np.float64)
        ext = float(np.linalg.norm(hi - lo))
        # object 0's transform turns the mesh about the origin: light and camera stand where the turned centre and normal are
        m = np.array(ra.transform_from_euler((0.0, 0.0, 0.0), (20.0, 35.0, 10.0))[:], dtype=np.float64).reshape(4, 4)
        c, n = np.asarray(centre, dtype=np.float64) @ m[:3, :3], np.asarray(normal, dtype=np.float64) @ m[:3, :3]
        return two_level_scene(pos, idx, _sheet_lights(c, n, 1.0)), _sheet_camera(c, n, 1.0, aspect), "wide2"
    if "offset_" in name or name.startswith("layers_"):
        scene = single_mesh_scene(pos, idx, _sheet_lights(centre, normal, 1.0, point=not name.startswith("sun_"), low=name.startswith("layers_")))
        return scene, _sheet_camera(centre, normal, 1.0, aspect), served_by(scene)
    s = ra.Scene()
    mat = s.add_material("diffuse", (0.7, 0.6, 0.5))
    if name.startswith("rect_"):
        k = 0 if "far" in name else int(name.split("_")[-1])
        y = ROOM_HEIGHT + 0.05 if "far" in name else ulps(ROOM_HEIGHT, -k if "below" in name else k)
        pos, idx = room_mesh()
        add_mesh(s, pos, idx, mat)
        s.add_area_light("rect", [0.3, 0.3], (30.0, 28.0, 25.0), ra.transform_from_euler((0.0, y, 0.0), (90.0, 0.0, 0.0)))
    else:
        floor, _ = sheet(16, 7)
        top = floor[np.argmax(floor[:, 1])]
        L = {"point_on_vertex": tuple(float(v) for v in top), "point_1ulp_behind_ceiling": (0.1, ulps(ROOM_HEIGHT, 1), -0.05), "point_homothetic": (0.1, 0.9, -0.05)}[name]
        pos, idx = room_mesh(L if name == "point_homothetic" else None)
        add_mesh(s, pos, idx, mat)
        s.add_point_light((6.0, 5.5, 5.0), ra.transform_from_euler(L, (0.0, 0.0, 0.0)))
    if name not in ALL_OCCLUDED:
        s.add_background_light((0.2, 0.3, 0.4))
    s.build()
    return s, _room_camera(aspect), served_by(s)


def served_by(scene):
    """the walk that serves the scene with the counters off: the one-level 4-wide walk for a scene whose one object is a mesh with a grid, the two-level one
    for several objects of which one is such a mesh, else the binary walk"""
    if not scene_grid(scene)[3]:
        return "binary"
    return "wide" if scene.desc.contents.numObjects == 1 else "wide2"


def mesh_objects(scene):
    """indices of the scene's mesh objects (Scene::BuildBVH orders the objects its own way)"""
    d = scene.desc.contents
    return [i for i in range(d.numObjects) if d.objects[i].shapeKind == 3 and d.objects[i].objectKind == 0]


def two_level_rays(scene, pos, seed=6, n=NUM_RAYS):
    """For two_level_scene: aimed(1.5) at either mesh object in world space (the second stands 1e3 extents away: its local rays come through invTransform
    at that magnitude), and rays from around the first up towards the far sphere."""
    rng = np.random.RandomState(seed)
    d = scene.desc.contents
    O, D = [], []
    part = n // 3
    for obj in mesh_objects(scene):
        m = np.array(d.objects[obj].transform[:], dtype=np.float64).reshape(4, 4)
        world = pos.astype(np.float64) @ m[:3, :3] + m[3, :3]
        tgt, ext = _targets(world, rng, part)
        u = _unit(rng, part)
        O.append(tgt - u * 1.5 * ext * rng.uniform(0.2, 1.0, (part, 1)))
        D.append(u)
    rest = n - 2 * part
    u = _unit(rng, rest)
    u[:, 1] = np.abs(u[:, 1])
    O.append(rng.uniform(-1.0, 1.0, (rest, 3)))
    D.append(u)
    return with_max_distance(scene, np.concatenate(O), np.concatenate(D), seed + 100)


# ---- the runner-up tolerance, per ray ------------------------------------------------------------------------------------------------------------
def fold_tolerance(rays, bound):
    """RT_WIDE_FOLD_TOL of each ray in float32: 2^-19 of the largest magnitude a slab test of the ray can produce (the m of trust_model)"""
    o, d = rays[:, 0:3].astype(F32), rays[:, 4:7].astype(F32)
    with np.errstate(all="ignore"):
        length = np.sqrt((d * d).sum(axis=1, dtype=F32), dtype=F32)
        inv = F32(1.0) / (d * (F32(1.0) / length)[:, None])
        m = np.abs(o * inv) + np.asarray(bound, dtype=F32) * np.abs(inv)
    return m.max(axis=1) * F32(2.0 ** -19)


def layer_runner_up(pos, idx, rays, oblique):
    """For layers_mesh: every copy traced alone by the oracle gives the stack's candidates of a ray (the triangle test does not know the tree).  Returns
    (best, second: the two smallest hit distances over the copies, float32, inf where there is none; robust: both lie well inside their triangle --
    barycentrics and their complement > 0.05 -- under a ray at least 17 degrees off the sheets, so that they pass their leaf boxes in any tree)."""
    nv, nt = len(pos) // LAYER_SHEETS, len(idx) // LAYER_SHEETS
    unbounded = np.array(rays, dtype=F32)
    unbounded[:, 3] = np.inf
    t = np.full((len(rays), LAYER_SHEETS), np.inf, dtype=F32)
    inside = np.zeros((len(rays), LAYER_SHEETS), dtype=bool)
    for s in range(LAYER_SHEETS):
        one = single_mesh_scene(pos[s * nv:(s + 1) * nv], idx[:nt])
        hits, _, _ = shim.closest(one.desc, unbounded, surfaces=False)
        hit = hits[:, 1] != ra.RT_INVALID_OBJECT
        u, v = hits[:, 3].view(F32), hits[:, 4].view(F32)
        t[hit, s] = hits[hit, 0].view(F32)
        inside[:, s] = hit & (u > 0.05) & (v > 0.05) & (u + v < 0.95)
    order = np.argsort(t, axis=1, kind="stable")
    i = np.arange(len(rays))
    d = rays[:, 4:7].astype(np.float64)
    cosine = np.abs(d @ layers_frame(oblique)[0]) / np.linalg.norm(d, axis=1)
    return t[i, order[:, 0]], t[i, order[:, 1]], inside[i, order[:, 0]] & inside[i, order[:, 1]] & (cosine > 0.3)


def must_retrace(scene, pos, idx, rays, oblique):
    """(must, band): trusted rays whose runner-up lies clearly within tol of their best hit -- the 4-wide walk may not decide them itself -- and those of
    them whose runner-up is farther than tol / 4: the rays a tolerance four times too narrow would decide."""
    base, step, bound, _ = scene_grid(scene)
    trusted, _, _ = trust_model(rays, base, step, bound)
    tol = fold_tolerance(rays, bound).astype(np.float64)
    best, second, robust = layer_runner_up(pos, idx, rays, oblique)
    with np.errstate(invalid="ignore"):
        gap = second.astype(np.float64) - best.astype(np.float64)
        must = trusted & robust & np.isfinite(second) & (gap <= (1.0 - BAND) * tol)
        return must, must & (gap > 0.3 * tol)
