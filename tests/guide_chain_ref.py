"""What the guide-chain tests share (tests/test_guide_chain_cpu.py, tests/test_gpu_guide_chain.py): the rule of include/rtgpu.h ("Guide chains") as a fold over
an oracle path recording, the two 70 x 37 scenes, and the oracle's recording of every pixel of pass 0 -- computed once per (scene, variant) and left unchanged."""
import ctypes as C

import numpy as np

import aov_ref
import oracle_lib
import path_records_ref
import scene_zoo
import raytracer_amd as ra
from raytracer_amd import scenes

W, H = aov_ref.W, aov_ref.H
SEED = 77
MAX_RAY_DEPTH = 6
NO_ROULETTE = 64   # minRussianRouletteDepth of the plain variants: deeper than any path here
INVALID_OBJECT, LIGHT_OBJECT, NO_MATERIAL = 0xFFFFFFFF, 0xFFFFFFFE, 0xFFFFFFFF
EV_SPECULAR_REFLECTION, EV_SPECULAR_REFRACTION, EV_SPECULAR = 16, 32, 48
# RtBsdf of the materials a chain passes through
PASSING_BSDFS = tuple(ra.BSDF_NAMES.index(n) for n in ("dielectric", "roughDielectric", "metal", "roughMetal"))
PLASTIC_BSDFS = tuple(ra.BSDF_NAMES.index(n) for n in ("plastic", "roughPlastic"))

_cache = {}


# ---- the scenes ------------------------------------------------------------------------------------------------------------------------------
def _hall():
    """The Sponza-class atrium (2000 triangles) seen along its nave: a smooth-metal mirror ahead and a second one facing it behind the camera (chains of two and
    more, up to the depth limit), a third above the first, tilted up so that it shows the rect light and the open sky, a glass sphere, a plastic and a rough-metal
    box.  Rect sizes are half extents."""
    pos, idx, nrm, tan, uv, mat = scenes.sponza_class_mesh(2000, seed=5)
    s = ra.Scene()
    mats = [s.add_material("diffuse", c) for _, c in scenes.SPONZA_MATERIALS]
    s.add_mesh(pos, idx, nrm, tan, uv, mat, mats)
    mirror = s.add_material("metal", (0.95, 0.9, 0.8))
    glass = s.add_material("dielectric", (0.9, 1.0, 0.95))
    plastic = s.add_material("plastic", (0.8, 0.2, 0.2))
    rough = s.add_material("roughMetal", (0.9, 0.8, 0.6), roughness=0.3)
    s.add_rect((4.5, 3.2), ra.transform_from_euler((-3.6, 3.3, 0.0), (0.0, -90.0, 0.0)), mirror)     # ahead, facing the camera
    s.add_rect((5.5, 3.6), ra.transform_from_euler((-14.6, 3.6, 0.3), (0.0, 90.0, 0.0)), mirror)    # behind the camera, facing the first
    s.add_rect((2.0, 1.5), ra.transform_from_euler((-4.0, 7.4, 1.5), (-30.0, -90.0, 0.0)), mirror)    # tilted up: the light and the sky
    s.add_sphere(1.1, ra.transform_from_euler((-6.5, 1.3, 3.0)), glass)
    s.add_box((0.9, 0.9, 0.9), ra.transform_from_euler((-5.0, 0.9, -0.6), (0.0, 25.0, 0.0)), plastic)
    s.add_box((0.7, 1.2, 0.7), ra.transform_from_euler((-6.5, 1.2, -3.0), (0.0, 30.0, 0.0)), rough)
    s.add_area_light("rect", [1.2, 1.2], (30.0, 28.0, 25.0), ra.transform_from_euler((-4.0, 11.0, 2.6), (90.0, 0.0, 0.0)))
    s.add_background_light((1.0, 1.5, 2.0))
    s.build()
    return s


def _textured():
    """scene_zoo.textured_scene and one smooth-metal rect in front of its normal-mapped mesh, turned so that it shows the mesh and the rect light.  The mirror's
    material has a normal map of its own: a light seen in it is evaluated with that material still in IntersectionData::material (the stale-material rule)"""
    s, _ = scene_zoo.textured_scene(W / H, triangles=2000)
    bumps = s.add_bitmap_texture(np.random.RandomState(3).uniform(0.42, 0.58, size=(8, 8, 4)).astype(np.float32), "R32G32B32A32_Float", filter="bilinear")
    mirror = s.add_material("metal", (0.95, 0.9, 0.8))
    s.set_material_texture(mirror, "normal", bumps, 0.6)
    s.add_rect((2.4, 1.8), ra.transform_from_euler((-4.0, 4.5, 0.3), (-54.0, -90.0, 0.0)), mirror)
    s.build()
    return s


def camera(lens=False):
    cam = ra.Camera((-12.5, 2.5, 0.3), (-6.0, 88.0, 0.0), W / H, 75.0)
    if lens:   # aov_ref.camera(lens=True)'s settings: depth of field on, hexagon bokeh, variable barrel distortion
        cam.set_dof(True, 9.0, 0.15)
        cam.set_lens(1, 0.01, 0.05)
    return cam


def scene(name):
    if ("scene", name) not in _cache:
        s = dict(hall=_hall, textured=_textured)[name]()
        bn = ra.load_blue_noise()
        s.desc.contents.blueNoise = bn.ctypes.data
        _cache["scene", name] = (s, bn)
    return _cache["scene", name][0]


def viewport_args(sampling_all=False, roulette=False):
    return dict(seed=SEED, max_ray_depth=MAX_RAY_DEPTH, min_russian_roulette_depth=0 if roulette else NO_ROULETTE, light_sampling_all=sampling_all)


def params(sampling_all=False, lens=False, roulette=False, skip=0):
    """pass `skip` of the frame's sample sequence, drawn from a viewport without a renderer (the sequence depends on the seed alone)"""
    vp = ra.Viewport(W, H, **viewport_args(sampling_all, roulette))
    vp.reset()
    cam = camera(lens)
    for _ in range(skip):
        vp.next_pass_params(cam)
    return vp.next_pass_params(cam)


def viewport(name, sampling_all=False, roulette=False, **renderer):
    vp = ra.Viewport(W, H, **viewport_args(sampling_all, roulette))
    vp.set_renderer(scene(name), **renderer)
    return vp


def oracle_frame(name, sampling_all=False, lens=False, roulette=False):
    """[vertices (n, 28)] for every pixel of pass 0, row by row -- the oracle's PathDebugData hook, as path_records_ref.oracle_frame takes it"""
    key = ("frame", name, sampling_all, lens, roulette)
    if key not in _cache:
        p = params(sampling_all, lens, roulette)
        desc = scene(name).desc
        _cache[key] = [oracle_lib.render_pixel_paths(desc, p, W, H, x, y, capacity=MAX_RAY_DEPTH + 2) for x, y in path_records_ref.all_pixels(W, H)]
    return _cache[key]


# ---- the rule ----------------------------------------------------------------------------------------------------------------------------------
def material_of(vertex, desc):
    """the material index of a recorded surface vertex: RtObject.materialIndex, or the triangle's for a mesh (NO_MATERIAL there: the object's)"""
    obj = desc.objects[int(vertex[6:7].view(np.uint32)[0])]
    if obj.objectKind == 0 and obj.shapeKind == 3:
        mesh = desc.meshes[obj.meshIndex]
        indices = C.cast(desc.vertexIndices, C.POINTER(C.c_uint32))
        m = indices[4 * (mesh.firstTriangle + int(vertex[7:8].view(np.uint32)[0])) + 3]
        if m != NO_MATERIAL:
            return int(m)
    return int(obj.materialIndex)


def is_surface(vertex):
    obj, sub = vertex[6:8].view(np.uint32)
    return obj != INVALID_OBJECT and sub != LIGHT_OBJECT


def fold(vertices, desc, max_chain):
    """include/rtgpu.h, "Guide chains", over an (n, 28) recording: (k, distance, throughput) -- the guide vertex's index, the np.float32 left-to-right sum of the
    hit distances (word 8) of vertices 0..k, and the (3,) float32 throughput on arrival at it.  Vertex j is passed iff it is not the closing record, its
    event (word 26; the closing record's is stale and never read) is specular, its material's bsdf is one of PASSING_BSDFS and j < max_chain."""
    n = len(vertices)
    k = 0
    while k < n - 1 and k < max_chain:
        v = vertices[k]
        if not (int(v[26:27].view(np.uint32)[0]) & EV_SPECULAR) or desc.materials[material_of(v, desc)].bsdf not in PASSING_BSDFS:
            break
        k += 1
    distance = np.float32(vertices[0, 8])
    for j in range(1, k + 1):
        distance = np.float32(distance + vertices[j, 8])
    throughput = np.ones(3, dtype=np.float32) if k == 0 else vertices[k - 1, 22:25].copy()
    return k, distance, throughput


def folded_frame(frame, desc, max_chain):
    """the fold of every pixel: (k (P,) uint32, distance (P,) float32, throughput (P, 3) float32, guide vertices (P, 28) float32, stale (P, 28) bool) -- `stale`
    is path_records_ref.stale_mask's row for the guide vertex IN ITS PATH"""
    ks, ds, ts, vs, ms = [], [], [], [], []
    for vertices in frame:
        k, d, t = fold(vertices, desc, max_chain)
        ks.append(k); ds.append(d); ts.append(t); vs.append(vertices[k]); ms.append(path_records_ref.stale_mask(vertices, desc)[k])
    return np.array(ks, dtype=np.uint32), np.array(ds, dtype=np.float32), np.stack(ts), np.stack(vs), np.stack(ms)


def census(frame, desc, max_chain):
    """pixel counts of the cases the GPU comparison must not lose (tests/test_guide_chain_cpu.py says which and why)"""
    c = dict(pixels=len(frame), k1=0, k2=0, diffuse_behind_mirror=0, stopped_by_max_chain=0, miss_behind_mirror=0, light_behind_mirror=0, closed_by_depth=0,
             plastic_specular=0, sphere_reflection=0, sphere_refraction=0, closed_on_passing_surface=0)
    for vertices in frame:
        k, _, _ = fold(vertices, desc, max_chain)
        n = len(vertices)
        g = vertices[k]
        closing = k == n - 1
        c["k1"] += k >= 1
        c["k2"] += k >= 2
        bsdf = desc.materials[material_of(g, desc)].bsdf if is_surface(g) else None
        obj, sub = g[6:8].view(np.uint32)
        if k >= 1 and obj == INVALID_OBJECT:
            c["miss_behind_mirror"] += 1
        elif k >= 1 and sub == LIGHT_OBJECT:
            c["light_behind_mirror"] += 1
        elif k >= 1 and bsdf not in PASSING_BSDFS and bsdf not in PLASTIC_BSDFS:
            c["diffuse_behind_mirror"] += 1
        if bsdf in PASSING_BSDFS and not closing and k == max_chain and (int(g[26:27].view(np.uint32)[0]) & EV_SPECULAR):
            c["stopped_by_max_chain"] += 1
        if bsdf is not None and closing and k == MAX_RAY_DEPTH:
            c["closed_by_depth"] += 1
        if bsdf in PASSING_BSDFS and closing and k < min(max_chain, MAX_RAY_DEPTH):
            c["closed_on_passing_surface"] += 1   # ended by roulette, a zero throughput or a missing event
        for j, v in enumerate(vertices[:-1]):
            if not is_surface(v):
                continue
            b, event = desc.materials[material_of(v, desc)].bsdf, int(v[26:27].view(np.uint32)[0])
            if j <= k and b in PLASTIC_BSDFS and (event & EV_SPECULAR) and j == k:
                c["plastic_specular"] += 1
            if j < k and b == ra.BSDF_NAMES.index("dielectric"):
                c["sphere_reflection"] += event == EV_SPECULAR_REFLECTION
                c["sphere_refraction"] += event == EV_SPECULAR_REFRACTION
    return c


def chain_planes_as_words(got):
    """chain_length, chain_distance, chain_throughput of a render_aovs(chain=N) result as (P,) uint32, (P,) uint32 and (P, 3) uint32 words"""
    return (np.ascontiguousarray(got["chain_length"]).reshape(-1).astype(np.uint32), np.ascontiguousarray(got["chain_distance"]).reshape(-1).view(np.uint32),
            np.ascontiguousarray(got["chain_throughput"]).reshape(3, -1).T.copy().view(np.uint32))
