"""The denoiser's C ABI (include/rtgpu.h: rtgpu_filter_atrous, rtgpu_denoise, rtgpu_postprocess_from), the part that needs no GPU: the symbols, the
parameter block's layout, the checks that come before any device work, and the wrappers' own refusals.  The device side: tests/test_gpu_denoise.py."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("rtgpu_filter_atrous", "rtgpu_filter_atrous_async", "rtgpu_denoise", "rtgpu_denoise_async", "rtgpu_postprocess_from")
INVALID_ARGUMENT = -1


def test_symbols_are_exported_and_the_abi_version_stays(built):
    import raytracer_amd as ra
    lib = ra.rtgpu_lib()
    for name in ENTRIES:
        assert hasattr(lib, name), name
    assert lib.rtgpu_abi_version() == 3   # added functions: no bump


def test_the_parameter_block_is_32_bytes_and_mirrors_the_header(built):
    import raytracer_amd as ra
    assert C.sizeof(ra.RtDenoiseParams) == 32
    text = open(os.path.join(ROOT, "include", "rtgpu.h")).read()
    body = re.search(r"typedef struct RtDenoiseParams\s*\{(.*?)\} RtDenoiseParams;", text, flags=re.S).group(1)
    fields = re.findall(r"^\s*(uint32_t|float)\s+(\w+)(\[\d+\])?;", body, flags=re.M)
    assert [name for _, name, _ in fields] == [name for name, _ in ra.RtDenoiseParams._fields_]
    offset = 0
    for (ctype, name, array), (_, mirror) in zip(fields, ra.RtDenoiseParams._fields_):
        assert getattr(ra.RtDenoiseParams, name).offset == offset, name
        assert (mirror is C.c_float) == (ctype == "float") or array
        offset += 4 * (int(array[1:-1]) if array else 1)
    assert offset == 32
    assert int(re.search(r"#define RT_DENOISE_DEMODULATE (\d+)u", text).group(1)) == ra.RT_DENOISE_DEMODULATE == 1


def test_a_null_context_is_refused_before_anything_else(built):
    import raytracer_amd as ra
    lib = ra.rtgpu_lib()
    p, pp, post = ra.denoise_params(), ra.RtPassParams(), ra.RtPostprocessParams()
    a = np.zeros(64, dtype=np.float32)
    ptr = a.ctypes.data_as(C.c_void_p)
    w = h = C.c_uint32(2)
    assert lib.rtgpu_filter_atrous(None, C.byref(p), w, h, ptr, ptr, ptr, ptr, ptr, ptr) == INVALID_ARGUMENT and b"NULL" in lib.rtgpu_last_error()
    assert lib.rtgpu_filter_atrous_async(None, C.byref(p), w, h, ptr, ptr, ptr, ptr, ptr, ptr, None) == INVALID_ARGUMENT
    assert lib.rtgpu_denoise(None, C.byref(p), C.byref(pp), ptr) == INVALID_ARGUMENT and b"NULL" in lib.rtgpu_last_error()
    assert lib.rtgpu_denoise_async(None, C.byref(p), C.byref(pp), ptr, None) == INVALID_ARGUMENT
    assert lib.rtgpu_postprocess_from(None, C.byref(post), ptr, ptr) == INVALID_ARGUMENT
    assert lib.rtgpu_filter_atrous(None, None, w, h, None, None, None, None, None, None) == INVALID_ARGUMENT


def test_wrapper_refusals(built):
    """malformed arrays, a Camera in place of the params and the missing renderer, before any device is touched"""
    import raytracer_amd as ra
    from raytracer_amd import scenes
    h, w = 4, 6
    color, depth, plane = np.zeros((h, w, 3), dtype=np.float32), np.zeros((h, w), dtype=np.float32), np.zeros((3, h, w), dtype=np.float32)
    with pytest.raises(ValueError, match="albedo"):
        ra.atrous_filter(color, depth, plane, plane)
    with pytest.raises(ValueError, match="normal"):
        ra.atrous_filter(color, depth, plane[:, :, :5], plane, demodulate=False)
    with pytest.raises(ValueError, match="depth"):
        ra.atrous_filter(color, depth.astype(np.float64), plane, plane, demodulate=False)
    with pytest.raises(ValueError, match="color"):
        ra.atrous_filter(depth, depth, plane, plane, demodulate=False)
    _, camera = scenes.sphere_area_light(1.0)
    vp = ra.Viewport(16, 16, seed=1)
    with pytest.raises(TypeError, match="next_pass_params"):
        vp.denoise(camera)
    with pytest.raises(RuntimeError, match="set_renderer"):
        vp.denoise(ra.RtPassParams())
    with pytest.raises(ValueError, match="image"):
        vp.front_buffer_from(np.zeros((16, 16, 4), dtype=np.float32))
