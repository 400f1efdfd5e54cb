"""AOVs (rtgpu_render_aovs), the part that needs no GPU: the symbols, the plane table against the header, the argument checks that come before any
device work, the Python wrapper's own checks, and -- oracle only -- that the frame the device tests use holds every kind of first hit.
The device side: tests/test_gpu_aovs.py."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def header_planes():
    """[(name, channels, 'f32' | 'u32')] in the order of enum RtAovPlane, and the value RT_AOV_NUM_PLANES gets"""
    text = open(os.path.join(ROOT, "include", "rtgpu.h")).read()
    body = re.search(r"typedef enum RtAovPlane \{(.*?)\} RtAovPlane;", text, flags=re.S).group(1)
    planes = []
    for line in body.splitlines()[1:]:
        names = [n for n in re.findall(r"RT_AOV_(\w+)", line) if n != "NUM_PLANES"]
        kind = re.search(r"/\* (\d) (f32|u32)", line)
        if names:
            assert kind, line
            planes += [(n.lower(), int(kind.group(1)), kind.group(2)) for n in names]
    assert body.split()[-1] == "RT_AOV_NUM_PLANES"   # the last enumerator: its value is the number of planes before it
    return planes, len(planes)


def test_symbols_are_exported_and_the_abi_version_stays(built):
    import raytracer_amd as ra
    lib = ra.rtgpu_lib()
    assert hasattr(lib, "rtgpu_render_aovs") and hasattr(lib, "rtgpu_render_aovs_async")
    assert lib.rtgpu_abi_version() == 3   # added functions: no bump


def test_plane_table_agrees_with_the_header(built):
    import raytracer_amd as ra
    planes, num = header_planes()
    assert num == 19 and len(ra.AOV_PLANES) == num
    assert list(ra.AOV_PLANES) == [name for name, _, _ in planes]
    for index, (name, channels, kind) in enumerate(planes):
        assert ra.AOV_PLANES[name] == (index, channels, np.float32 if kind == "f32" else np.uint32), name
    assert ra.AOV_PLANES["depth"][0] == 0 and ra.AOV_PLANES["triangle_tests_passed"][0] == num - 1


def test_argument_checks_without_a_device(built):
    """a NULL context comes before anything else (RTGPU_ERR_INVALID_ARGUMENT = -1), with a message -- even for an empty request"""
    import raytracer_amd as ra
    lib = ra.rtgpu_lib()
    p = ra.RtPassParams()
    planes = (C.c_uint32 * 1)(0)
    plane = np.zeros(4, dtype=np.float32)
    outputs = (C.c_void_p * 1)(plane.ctypes.data)
    for call in (lib.rtgpu_render_aovs, lambda *a: lib.rtgpu_render_aovs_async(*a, None)):
        assert call(None, C.byref(p), planes, C.c_uint32(1), outputs) == -1
        assert b"NULL" in lib.rtgpu_last_error()
        assert call(None, None, None, C.c_uint32(0), None) == -1


def test_wrapper_refusals(built):
    """an unknown plane, a Camera in place of the params, and -- with well-formed arguments -- the missing renderer, before any device is touched"""
    import raytracer_amd as ra
    from raytracer_amd import scenes
    _, camera = scenes.sphere_area_light(1.0)
    vp = ra.Viewport(16, 16, seed=1)
    with pytest.raises(ValueError, match="albedo"):
        vp.render_aovs(ra.RtPassParams(), planes=("depth", "albedo"))
    with pytest.raises(TypeError, match="next_pass_params"):
        vp.render_aovs(camera)
    with pytest.raises(RuntimeError, match="set_renderer"):
        vp.render_aovs(ra.RtPassParams(), planes=("depth",))
    with pytest.raises(RuntimeError, match="set_renderer"):
        vp.render_aovs(ra.RtPassParams(), planes="depth", device=True)


@pytest.mark.parametrize("name, lens", [("mixed", False), ("mixed", True), ("textured", False)])
def test_the_device_tests_frame_holds_every_kind_of_first_hit(built, name, lens):
    """Oracle only: misses, finite-light hits, mesh triangles and analytic shapes are all in the 70 x 37 frame, every pixel's primary ray is one ray, and the
    words the device test masks (what the reference leaves unwritten in a first vertex) are a small part of what it compares."""
    import aov_ref as ref
    vertices = ref.oracle_first_vertices(name, lens)
    assert vertices.shape == (ref.W * ref.H, 28)
    classes = ref.hit_classes(name, vertices)
    print(name, lens, [int(c.sum()) for c in classes])
    assert all(c.sum() >= 10 for c in classes) and sum(int(c.sum()) for c in classes) == ref.W * ref.H
    assert np.isposinf(vertices[classes[0], 8]).all()
    stale = ref.stale_words(name, vertices)[:, 6:22]
    assert stale.sum() * 10 < stale.size
    if not lens:
        counters = ref.oracle_pixel_counters(name)
        assert (counters[..., 0] == 1).all()          # numRays: the primary ray and nothing else
        assert (counters[..., 4] > 0).any() and (counters[..., 7] > 0).any()
