"""Path records (rtgpu_record_paths), the part that needs no GPU: the symbol, the struct layouts, the argument checks that come before any
device work, and the Python wrapper's own checks.  The device side: tests/test_gpu_path_records.py."""
import ctypes as C

import numpy as np
import pytest


def test_symbol_is_exported_and_the_abi_version_stays(built):
    import raytracer_amd as ra
    lib = ra.rtgpu_lib()
    assert hasattr(lib, "rtgpu_record_paths")
    assert lib.rtgpu_abi_version() == 3   # an added function: no bump


def test_struct_sizes(built):
    import raytracer_amd as ra
    assert C.sizeof(ra.RtPathVertex) == 112
    assert C.sizeof(ra.RtPathInfo) == 32
    assert ra.RtPathInfo.radiance.offset == 8
    assert ra.PATH_TERMINATION_REASONS[1] == "HitBackground" and ra.PATH_TERMINATION_REASONS[6] == "RussianRoulette" and len(ra.PATH_TERMINATION_REASONS) == 7


def test_argument_checks_without_a_device(built):
    """NULL context / NULL params come before anything else (RTGPU_ERR_INVALID_ARGUMENT = -1), with a message."""
    import raytracer_amd as ra
    lib = ra.rtgpu_lib()
    p = ra.RtPassParams()
    xy = (C.c_uint32 * 2)(0, 0)
    v = (ra.RtPathVertex * 4)()
    info = ra.RtPathInfo()
    assert lib.rtgpu_record_paths(None, C.byref(p), xy, C.c_uint32(1), C.c_uint32(4), v, C.byref(info)) == -1
    assert b"NULL" in lib.rtgpu_last_error()
    assert lib.rtgpu_record_paths(None, None, xy, C.c_uint32(1), C.c_uint32(4), v, C.byref(info)) == -1
    assert lib.rtgpu_record_paths(None, C.byref(p), None, C.c_uint32(0), C.c_uint32(4), None, None) == -1   # even an empty call needs a context


@pytest.mark.parametrize("pixels", [
    [(1, 2, 3)],                                  # not pairs
    [1, 2],                                       # a flat list
    [(0.5, 1.0)],                                 # not integers
    [(-1, 0)],                                    # negative
    [(16, 0)], [(0, 16)],                         # outside the 16 x 16 frame
    np.zeros((2, 2, 2), dtype=np.int32),          # too many dimensions
])
def test_wrapper_refuses_malformed_pixel_lists(built, pixels):
    """... before it reaches the library: the viewport below has no renderer, and the complaint is about the pixels."""
    import raytracer_amd as ra
    vp = ra.Viewport(16, 16, seed=1)
    with pytest.raises(ValueError, match="pixel"):
        vp.record_paths(ra.RtPassParams(), pixels)


def test_wrapper_refuses_a_camera_and_a_zero_capacity(built):
    import raytracer_amd as ra
    from raytracer_amd import scenes
    _, camera = scenes.sphere_area_light(1.0)
    vp = ra.Viewport(16, 16, seed=1)
    with pytest.raises(TypeError, match="next_pass_params"):
        vp.record_paths(camera, [(0, 0)])
    with pytest.raises(ValueError, match="max_vertices"):
        vp.record_paths(ra.RtPassParams(), [(0, 0)], max_vertices=0)
    with pytest.raises(RuntimeError, match="set_renderer"):   # well-formed arguments get as far as the missing renderer
        vp.record_paths(ra.RtPassParams(), [(0, 0)])


@pytest.mark.parametrize("name", ["box_mesh", "cornell", "mesh_2k_all", "mesh_single"])
def test_stale_fields_are_a_minority_of_the_compared_words(built, name):
    """The device test masks the fields the reference leaves stale (path_records_ref.stale_mask).  On each of its fixtures that mask covers
    less than half of the recorded words (a miss alone loses 14 of its 28), and the fixture has what it was chosen for: paths that end on the
    background or on a light, on a surface, and at the depth limit.  Oracle only."""
    import path_records_ref as ref
    scene, _, w, h, args = ref.fixture(name)
    frame = ref.oracle_frame(name)
    assert len(frame) == w * h
    masked = sum(int(ref.stale_mask(v, scene.desc.contents).sum()) for v, _ in frame)
    words = sum(v.size for v, _ in frame)
    print("%s: %d paths, %d vertices, %d of %d words masked (%.1f %%)" % (name, len(frame), words // 28, masked, words, 100.0 * masked / words))
    assert masked * 2 < words
    assert max(len(v) for v, _ in frame) == args["max_ray_depth"] + 1          # a path that reaches the depth limit
    last_objects = np.array([v[-1, 6:8].view(np.uint32) for v, _ in frame])
    assert (last_objects[:, 0] != ref.INVALID_OBJECT).any()                     # a path that ends on a surface
    assert ((last_objects[:, 0] == ref.INVALID_OBJECT) | (last_objects[:, 1] == ref.LIGHT_OBJECT)).any()   # and one that leaves the scene or finds the light
