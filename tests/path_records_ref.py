"""What the path-record tests share: the oracle's recording of a whole fixture frame (computed once per fixture and left unchanged) and the mask
of the fields the reference leaves stale (include/rtgpu.h, rtgpu_record_paths: the device writes zero there)."""
import numpy as np

import oracle_lib
import ref_scenes
import raytracer_amd as ra

# the four fixtures of tests/test_gpu_path_records.py: between them every hit kind (miss, sphere, box, rect, area-light hit, mesh triangle with
# interpolated tangents) and paths up to the depth limit
FIXTURE_NAMES = ("box_mesh", "cornell", "mesh_2k_all", "mesh_single")
INVALID_OBJECT, LIGHT_OBJECT = 0xFFFFFFFF, 0xFFFFFFFE

_fixtures = {}
_oracle = {}


def fixture(name):
    """(scene, camera, width, height, viewport arguments) of a ref_scenes fixture, with its own depth, dimensions and light mode; built once"""
    if name not in _fixtures:
        make, w, h, _, depth, sampling_all, dims = ref_scenes.FIXTURES[name]
        scene, camera = make(w / h)
        bn = ra.load_blue_noise()
        scene.desc.contents.blueNoise = bn.ctypes.data
        _fixtures[name] = (scene, camera, w, h, dict(seed=ref_scenes.SEED, max_ray_depth=depth, dimensions=dims, light_sampling_all=sampling_all), bn)
    return _fixtures[name][:5]


def first_pass_params(name):
    """the fixture's pass 0, drawn from a viewport without a renderer (the sample sequence depends on the seed alone)"""
    scene, camera, w, h, args = fixture(name)
    vp = ra.Viewport(w, h, **args)
    vp.reset()
    return vp.next_pass_params(camera)


def all_pixels(w, h):
    return [(x, y) for y in range(h) for x in range(w)]


def oracle_frame(name):
    """[(vertices (n, 28), radiance (3,))] for every pixel of the fixture's pass 0, row by row -- the oracle's PathDebugData hook"""
    if name not in _oracle:
        scene, _, w, h, args = fixture(name)
        p = first_pass_params(name)
        out = []
        for x, y in all_pixels(w, h):
            v = oracle_lib.render_pixel_paths(scene.desc, p, w, h, x, y, capacity=args["max_ray_depth"] + 2)
            out.append((v, oracle_lib.render_pixel(scene.desc, p, w, h, x, y)[:3].copy()))
        _oracle[name] = out
    return _oracle[name]


def stale_mask(vertices, desc):
    """(n, 28) bool: the words of a path's records that the reference leaves as an earlier vertex wrote them.  Exactly the list of
    include/rtgpu.h: word 27; word 26 of the closing record; on a miss word 7 and words 9..21; on a hit that is not a mesh triangle words 9, 10."""
    m = np.zeros(vertices.shape, dtype=bool)
    m[:, 27] = True
    m[-1, 26] = True
    objects = vertices[:, 6].view(np.uint32)
    miss = objects == INVALID_OBJECT
    m[miss, 7] = True
    m[miss, 9:22] = True
    triangle = np.array([(not ms) and desc.objects[int(o)].objectKind == 0 and desc.objects[int(o)].shapeKind == 3 for ms, o in zip(miss, objects)], dtype=bool)
    m[~triangle, 9:11] = True
    return m
