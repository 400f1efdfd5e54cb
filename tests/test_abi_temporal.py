"""The C ABI of temporal accumulation (include/rtgpu.h: rtgpu_temporal_accumulate, rtgpu_denoise_temporal, rtgpu_temporal_reset), the part that needs no
GPU: the symbols, the parameter block's layout, the checks that come before any device work, and the wrappers' own refusals.  The device side:
tests/test_gpu_temporal.py."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("rtgpu_temporal_accumulate", "rtgpu_temporal_accumulate_async", "rtgpu_denoise_temporal", "rtgpu_denoise_temporal_async", "rtgpu_temporal_reset")
FIELDS = ["flags", "colorScale", "alphaMin", "maxHistory", "normalThreshold", "planeTolerance", "prevSampleOffset", "prevWorldToScreen"]
INVALID_ARGUMENT = -1


def test_symbols_are_exported_and_the_abi_version_stays(built):
    import raytracer_amd as ra
    lib = ra.rtgpu_lib()
    for name in ENTRIES:
        assert hasattr(lib, name), name
    assert lib.rtgpu_abi_version() == 3   # added functions: no bump
    text = open(os.path.join(ROOT, "include", "rtgpu.h")).read()
    assert int(re.search(r"#define RTGPU_ABI_VERSION (\d+)u", text).group(1)) == 3
    for name in ENTRIES:
        assert re.search(r"\bint %s\(" % name, text), name


def test_the_parameter_block_is_96_bytes_and_mirrors_the_header(built):
    import raytracer_amd as ra
    assert C.sizeof(ra.RtTemporalParams) == 96
    text = open(os.path.join(ROOT, "include", "rtgpu.h")).read()
    body = re.search(r"typedef struct RtTemporalParams\s*\{(.*?)\} RtTemporalParams;", text, flags=re.S).group(1)
    fields = re.findall(r"^\s*(uint32_t|float)\s+(\w+)(\[\d+\])?;", body, flags=re.M)
    assert [name for _, name, _ in fields] == [name for name, _ in ra.RtTemporalParams._fields_] == FIELDS
    offset = 0
    for (ctype, name, array), (_, mirror) in zip(fields, ra.RtTemporalParams._fields_):
        assert getattr(ra.RtTemporalParams, name).offset == offset, name
        assert C.sizeof(mirror) == 4 * (int(array[1:-1]) if array else 1), name
        assert (mirror is C.c_uint32) == (ctype == "uint32_t"), name
        offset += C.sizeof(mirror)
    assert offset == 96
    assert int(re.search(r"#define RT_DENOISE_INPUT_PREPARED (\d+)u", text).group(1)) == ra.RT_DENOISE_INPUT_PREPARED == 2
    # the wrappers' defaults are the header's
    p = ra.temporal_params()
    assert (p.flags, p.colorScale, p.maxHistory) == (1, 1.0, 64.0) and abs(p.alphaMin - 0.1) < 1e-7 and abs(p.normalThreshold - 0.9) < 1e-7 and abs(p.planeTolerance - 0.01) < 1e-8
    m = np.arange(16, dtype=np.float32).reshape(4, 4)
    p = ra.temporal_params(prev_world_to_screen=m, prev_sample_offset=(0.25, -0.5), demodulate=False)
    assert list(p.prevWorldToScreen) == list(range(16)) and list(p.prevSampleOffset) == [0.25, -0.5] and p.flags == 0


def test_a_null_context_is_refused_before_anything_else(built):
    import raytracer_amd as ra
    lib = ra.rtgpu_lib()
    t, v, pp = ra.temporal_params(), ra.denoise_var_params(), ra.RtPassParams()
    a = np.zeros(64, dtype=np.float32)
    ptr = a.ctypes.data_as(C.c_void_p)
    w = h = C.c_uint32(2)
    buffers = (ptr,) * 18
    assert lib.rtgpu_temporal_accumulate(None, C.byref(t), w, h, *buffers) == INVALID_ARGUMENT and b"NULL" in lib.rtgpu_last_error()
    assert lib.rtgpu_temporal_accumulate_async(None, C.byref(t), w, h, *(buffers + (None,))) == INVALID_ARGUMENT
    assert lib.rtgpu_denoise_temporal(None, C.byref(t), C.byref(v), C.byref(pp), ptr, ptr) == INVALID_ARGUMENT and b"NULL" in lib.rtgpu_last_error()
    assert lib.rtgpu_denoise_temporal_async(None, C.byref(t), None, C.byref(pp), ptr, None, None) == INVALID_ARGUMENT
    assert lib.rtgpu_temporal_reset(None) == INVALID_ARGUMENT


def test_wrapper_refusals(built):
    """malformed arrays, a history without its camera or with one id plane, and the missing renderer, before any device is touched"""
    import raytracer_amd as ra
    h, w = 4, 6
    color, depth, plane = np.zeros((h, w, 3), dtype=np.float32), np.zeros((h, w), dtype=np.float32), np.zeros((3, h, w), dtype=np.float32)
    ids = np.zeros((h, w), dtype=np.uint32)
    history = dict(a=color, b=color, length=depth, depth=depth, normal=plane, position=plane, object_id=None)
    with pytest.raises(ValueError, match="albedo"):
        ra.temporal_accumulate(color, color, depth, plane, plane)
    with pytest.raises(ValueError, match="normal"):
        ra.temporal_accumulate(color, color, depth, plane[:, :, :5], plane, demodulate=False)
    with pytest.raises(ValueError, match="object_id"):
        ra.temporal_accumulate(color, color, depth, plane, plane, demodulate=False, object_id=ids.astype(np.int64))
    with pytest.raises(ValueError, match="prev_world_to_screen"):
        ra.temporal_accumulate(color, color, depth, plane, plane, demodulate=False, history=history)
    with pytest.raises(ValueError, match="both id planes"):
        ra.temporal_accumulate(color, color, depth, plane, plane, demodulate=False, object_id=ids, history=history, prev_world_to_screen=np.eye(4))
    with pytest.raises(ValueError, match="prev_length"):
        ra.temporal_accumulate(color, color, depth, plane, plane, demodulate=False, history=dict(history, length=plane), prev_world_to_screen=np.eye(4))
    with pytest.raises(ValueError, match="history"):
        ra.temporal_accumulate(color, color, depth, plane, plane, demodulate=False, history=dict(a=color), prev_world_to_screen=np.eye(4))
    with pytest.raises(ValueError, match="color_half"):
        ra.atrous_filter(color, depth, plane, plane, demodulate=False, prepared=True)
    vp = ra.Viewport(16, 16, seed=1)
    with pytest.raises(RuntimeError, match="set_renderer"):
        vp.denoise(ra.RtPassParams(), temporal=True)
    with pytest.raises(ValueError, match="return_variance"):
        vp.denoise(ra.RtPassParams(), temporal=True, variance=False, return_variance=True)
    vp.reset_history()   # (no renderer: nothing to drop)
