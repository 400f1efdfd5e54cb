"""What the AOV tests share (tests/test_gpu_aovs.py): the 70 x 37 frame, its scenes and cameras, and the oracle's answers for every pixel -- first path
vertices, Debug renderer colours, per-pixel counters -- each computed once and left unchanged."""
import ctypes as C

import numpy as np

import oracle_lib
import path_records_ref
import scene_zoo
import raytracer_amd as ra

# not a multiple of 64 wide, 2590 pixels = 10 blocks of 256 and a part of one, two 64 x 64 tiles across
W, H = 70, 37
SEED = 77
INVALID_OBJECT, LIGHT_OBJECT, NO_MATERIAL = 0xFFFFFFFF, 0xFFFFFFFE, 0xFFFFFFFF
GEOMETRY_PLANES = ("object_id", "sub_object_id", "depth", "barycentrics", "position", "normal", "tangent", "texcoord")
MATERIAL_PLANES = ("base_color", "emission", "roughness", "metalness", "ior")
COST_PLANES = ("box_tests", "box_tests_passed", "triangle_tests", "triangle_tests_passed")
ALL_PLANES = tuple(ra.AOV_PLANES)
# DebugRenderingMode (include/rtgpu.h) -> how the mode's colour follows from the raw planes
DEBUG_MODES = dict(position=3, normal=4, tangent=5, bitangent=6, base_color=8, emission=9, roughness=10, metalness=11, ior=12)

_cache = {}


def _scene(name):
    """(scene, camera): the zoo's mesh scenes seen from inside the atrium, looking up far enough for the open roof (misses) and the rect light above it"""
    if ("scene", name) not in _cache:
        if name == "mixed":       # a mesh, a sphere and a box, a finite area light, a background light
            scene, _ = scene_zoo.mesh_scene(W / H, triangles=2000)
        elif name == "textured":  # base-colour bitmaps, normal maps, roughness / metalness / emission textures on the mesh and the analytic shapes
            scene, _ = scene_zoo.textured_scene(W / H, triangles=2000)
        else:
            raise KeyError(name)
        bn = ra.load_blue_noise()
        scene.desc.contents.blueNoise = bn.ctypes.data
        _cache["scene", name] = (scene, bn)
    return _cache["scene", name][0]


def camera(lens=False):
    cam = ra.Camera((-7.0, 1.0, 0.4), (-40.0, 88.0, 0.0), W / H, 75.0)
    if lens:   # depth of field on, hexagon bokeh, variable barrel distortion
        cam.set_dof(True, 9.0, 0.15)
        cam.set_lens(1, 0.01, 0.05)
    return cam


def scene(name):
    return _scene(name)


def params(lens=False, skip=0):
    """pass `skip` of the frame's sample sequence, drawn from a viewport without a renderer (the sequence depends on the seed alone)"""
    vp = ra.Viewport(W, H, seed=SEED, max_ray_depth=0)
    vp.reset()
    cam = camera(lens)
    for _ in range(skip):
        vp.next_pass_params(cam)
    return vp.next_pass_params(cam)


def viewport(name, **renderer):
    vp = ra.Viewport(W, H, seed=SEED, max_ray_depth=0)
    vp.set_renderer(scene(name), **renderer)
    return vp


def oracle_first_vertices(name, lens):
    """(H * W, 28) float32: the first vertex of every pixel's path, row by row (oracle_lib.render_pixel_paths with maxRayDepth = 0)"""
    key = ("vertices", name, lens)
    if key not in _cache:
        p = params(lens)
        assert p.maxRayDepth == 0
        desc = scene(name).desc
        rows = []
        for y in range(H):
            for x in range(W):
                v = oracle_lib.render_pixel_paths(desc, p, W, H, x, y, capacity=2)
                assert len(v) == 1
                rows.append(v[0])
        _cache[key] = np.stack(rows)
    return _cache[key]


def oracle_debug_colors(name):
    """plane name -> (H, W, 3) float32: one Debug pass per mode onto a zero film"""
    key = ("debug", name)
    if key not in _cache:
        p = params()
        out = {}
        for plane, mode in DEBUG_MODES.items():
            film = np.zeros((H, W, 3), dtype=np.float32)
            oracle_lib.render_pass_debug(scene(name).desc, p, W, H, mode, film)
            out[plane] = film
        _cache[key] = out
    return _cache[key]


def oracle_pixel_counters(name):
    """(H, W, 16) uint64: RtCounters of every pixel's primary ray alone (maxRayDepth = 0)"""
    key = ("counters", name)
    if key not in _cache:
        p = params()
        desc = scene(name).desc
        out = np.zeros((H, W, 16), dtype=np.uint64)
        rgba = (C.c_float * 4)()
        for y in range(H):
            for x in range(W):
                oracle_lib.lib().rto_render_pixel(desc, C.byref(p), C.c_uint32(W), C.c_uint32(H), C.c_uint32(x), C.c_uint32(y), rgba, out[y, x].ctypes.data_as(C.POINTER(C.c_uint64)))
        _cache[key] = out
    return _cache[key]


def hit_classes(name, vertices):
    """bool masks over the pixels: miss, finite light, mesh triangle, analytic shape"""
    desc = scene(name).desc.contents
    obj, sub = vertices[:, 6].view(np.uint32), vertices[:, 7].view(np.uint32)
    miss = obj == INVALID_OBJECT
    light = ~miss & (sub == LIGHT_OBJECT)
    mesh = np.array([(not m) and desc.objects[int(o)].objectKind == 0 and desc.objects[int(o)].shapeKind == 3 for m, o in zip(miss, obj)], dtype=bool)
    return miss, light, mesh, ~miss & ~light & ~mesh


def stale_words(name, vertices):
    """(H * W, 28) bool: the words of a first vertex the reference leaves unwritten (path_records_ref.stale_mask: the list of include/rtgpu.h), where the
    oracle's record holds whatever its stack held and the planes hold zero"""
    desc = scene(name).desc.contents
    return np.concatenate([path_records_ref.stale_mask(vertices[i:i + 1], desc) for i in range(len(vertices))])


def planes_as_vertex_words(a):
    """the geometry planes of a render_aovs result laid out as words 6..21 of RtPathVertex, (H * W, 16) uint32"""
    cols = [a["object_id"].reshape(1, -1), a["sub_object_id"].reshape(1, -1), a["depth"].reshape(1, -1), a["barycentrics"].reshape(2, -1), a["position"].reshape(3, -1),
            a["normal"].reshape(3, -1), a["tangent"].reshape(3, -1), a["texcoord"].reshape(2, -1)]
    return np.concatenate([np.ascontiguousarray(c).view(np.uint32) for c in cols]).T.copy()
