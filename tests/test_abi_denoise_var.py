"""The variance-guided denoiser's C ABI (include/rtgpu.h: rtgpu_filter_atrous_var, rtgpu_denoise_var and their _async siblings), the part that needs no
GPU: the symbols, the parameter block's layout, the checks that come before any device work, and the wrappers' own refusals.  The device side:
tests/test_gpu_denoise_var.py."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("rtgpu_filter_atrous_var", "rtgpu_filter_atrous_var_async", "rtgpu_denoise_var", "rtgpu_denoise_var_async")
INVALID_ARGUMENT = -1


def test_symbols_are_exported_and_the_abi_version_stays(built):
    import raytracer_amd as ra
    lib = ra.rtgpu_lib()
    for name in ENTRIES:
        assert hasattr(lib, name), name
    assert lib.rtgpu_abi_version() == 3   # added functions: no bump


def test_the_parameter_block_is_32_bytes_and_mirrors_the_header(built):
    import raytracer_amd as ra
    assert C.sizeof(ra.RtDenoiseVarParams) == 32
    text = open(os.path.join(ROOT, "include", "rtgpu.h")).read()
    body = re.search(r"typedef struct RtDenoiseVarParams\s*\{(.*?)\} RtDenoiseVarParams;", text, flags=re.S).group(1)
    fields = re.findall(r"^\s*(uint32_t|float)\s+(\w+);", body, flags=re.M)
    assert [name for _, name in fields] == [name for name, _ in ra.RtDenoiseVarParams._fields_] == [
        "iterations", "flags", "colorScale", "sigmaLum", "sigmaNormal", "sigmaPlane", "varianceFloor", "_pad"]
    for k, ((ctype, name), (_, mirror)) in enumerate(zip(fields, ra.RtDenoiseVarParams._fields_)):
        assert getattr(ra.RtDenoiseVarParams, name).offset == 4 * k, name
        assert (mirror is C.c_float) == (ctype == "float"), name
    p = ra.denoise_var_params()
    assert (p.iterations, p.flags, p.sigmaLum, p._pad) == (5, ra.RT_DENOISE_DEMODULATE, 4.0, 0) and p.varianceFloor == np.float32(1e-10)
    # the existing block and its defaults are as they were
    assert C.sizeof(ra.RtDenoiseParams) == 32 and ra.denoise_params().sigmaColor == 2.0


def test_a_null_context_is_refused_before_anything_else(built):
    import raytracer_amd as ra
    lib = ra.rtgpu_lib()
    p, pp = ra.denoise_var_params(), ra.RtPassParams()
    a = np.zeros(64, dtype=np.float32)
    ptr = a.ctypes.data_as(C.c_void_p)
    w = h = C.c_uint32(2)
    assert lib.rtgpu_filter_atrous_var(None, C.byref(p), w, h, ptr, ptr, ptr, ptr, ptr, ptr, ptr, ptr) == INVALID_ARGUMENT and b"NULL" in lib.rtgpu_last_error()
    assert lib.rtgpu_filter_atrous_var_async(None, C.byref(p), w, h, ptr, ptr, ptr, ptr, ptr, ptr, ptr, ptr, None) == INVALID_ARGUMENT
    assert lib.rtgpu_denoise_var(None, C.byref(p), C.byref(pp), ptr, ptr) == INVALID_ARGUMENT and b"NULL" in lib.rtgpu_last_error()
    assert lib.rtgpu_denoise_var_async(None, C.byref(p), C.byref(pp), ptr, ptr, None) == INVALID_ARGUMENT
    assert lib.rtgpu_filter_atrous_var(None, None, w, h, None, None, None, None, None, None, None, None) == INVALID_ARGUMENT
    assert lib.rtgpu_denoise_var(None, None, None, None, None) == INVALID_ARGUMENT


def test_wrapper_refusals(built):
    """malformed arrays and keyword combinations, before any device is touched"""
    import raytracer_amd as ra
    h, w = 4, 6
    color, depth, plane = np.zeros((h, w, 3), dtype=np.float32), np.zeros((h, w), dtype=np.float32), np.zeros((3, h, w), dtype=np.float32)
    with pytest.raises(ValueError, match="color_half"):
        ra.atrous_filter(color, depth, plane, plane, demodulate=False, return_variance=True)
    with pytest.raises(ValueError, match="color_half"):
        ra.atrous_filter(color, depth, plane, plane, demodulate=False, color_half=color[:, :5])
    with pytest.raises(ValueError, match="color_half"):
        ra.atrous_filter(color, depth, plane, plane, demodulate=False, color_half=color.astype(np.float64))
    with pytest.raises(ValueError, match="albedo"):
        ra.atrous_filter(color, depth, plane, plane, color_half=color)
    vp = ra.Viewport(16, 16, seed=1)
    with pytest.raises(ValueError, match="variance=True"):
        vp.denoise(ra.RtPassParams(), return_variance=True)
    with pytest.raises(RuntimeError, match="set_renderer"):
        vp.denoise(ra.RtPassParams(), variance=True)
