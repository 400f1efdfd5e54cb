"""The C ABI of history clipping (include/rtgpu.h: rtgpu_temporal_accumulate_clip, rtgpu_denoise_temporal_clip), the part that needs no GPU: the symbols, the
clip block's layout, the checks that come before any device work, and the wrappers' own refusals.  The device side: tests/test_gpu_temporal_clip.py."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("rtgpu_temporal_accumulate_clip", "rtgpu_temporal_accumulate_clip_async", "rtgpu_denoise_temporal_clip", "rtgpu_denoise_temporal_clip_async")
INVALID_ARGUMENT = -1


def test_symbols_are_exported_and_the_abi_version_stays(built):
    import raytracer_amd as ra
    lib = ra.rtgpu_lib()
    text = open(os.path.join(ROOT, "include", "rtgpu.h")).read()
    for name in ENTRIES:
        assert hasattr(lib, name), name
        assert re.search(r"\bint %s\(" % name, text), name
    assert lib.rtgpu_abi_version() == 3   # added functions: no bump


def test_the_clip_block_is_16_bytes_and_mirrors_the_header(built):
    import raytracer_amd as ra
    assert C.sizeof(ra.RtTemporalClip) == 16
    text = open(os.path.join(ROOT, "include", "rtgpu.h")).read()
    body = re.search(r"typedef struct RtTemporalClip\s*\{(.*?)\} RtTemporalClip;", text, flags=re.S).group(1)
    fields = re.findall(r"^\s*(uint32_t|float)\s+(\w+);", body, flags=re.M)
    assert [name for _, name in fields] == [name for name, _ in ra.RtTemporalClip._fields_] == ["radius", "gamma", "minCount", "_pad"]
    for k, ((ctype, name), (_, mirror)) in enumerate(zip(fields, ra.RtTemporalClip._fields_)):
        assert getattr(ra.RtTemporalClip, name).offset == 4 * k and C.sizeof(mirror) == 4 and (mirror is C.c_uint32) == (ctype == "uint32_t"), name
    # the wrapper's argument: None, True or a dict over the defaults
    assert ra.temporal_clip(None) is None
    d = ra.TEMPORAL_CLIP_DEFAULTS
    assert (d["radius"], d["min_count"]) == (3, 9) and 0.0 <= d["gamma"] <= 1e6
    c = ra.temporal_clip(True)
    assert (c.radius, c.gamma, c.minCount, c._pad) == (3, np.float32(d["gamma"]), 9, 0)
    c = ra.temporal_clip(dict(radius=1, gamma=0.5))
    assert (c.radius, c.gamma, c.minCount) == (1, 0.5, 9)
    for bad in (dict(sigma=1.0), 2.0, "on"):
        with pytest.raises(ValueError, match="clip"):
            ra.temporal_clip(bad)


def test_a_null_context_is_refused_before_anything_else(built):
    import raytracer_amd as ra
    lib = ra.rtgpu_lib()
    t, v, pp, clip = ra.temporal_params(), ra.denoise_var_params(), ra.RtPassParams(), ra.temporal_clip(True)
    a = np.zeros(64, dtype=np.float32)
    ptr = a.ctypes.data_as(C.c_void_p)
    w = h = C.c_uint32(2)
    buffers = (ptr,) * 18 + (None, C.c_uint32(0), C.byref(clip), ptr)
    assert lib.rtgpu_temporal_accumulate_clip(None, C.byref(t), w, h, *buffers) == INVALID_ARGUMENT and b"NULL" in lib.rtgpu_last_error()
    assert lib.rtgpu_temporal_accumulate_clip_async(None, C.byref(t), w, h, *(buffers + (None,))) == INVALID_ARGUMENT
    assert lib.rtgpu_denoise_temporal_clip(None, C.byref(t), C.byref(v), C.byref(pp), ptr, ptr, C.byref(clip), ptr) == INVALID_ARGUMENT and b"NULL" in lib.rtgpu_last_error()
    assert lib.rtgpu_denoise_temporal_clip_async(None, C.byref(t), None, C.byref(pp), ptr, None, None, None, None) == INVALID_ARGUMENT


def test_wrapper_refusals(built):
    import raytracer_amd as ra
    h, w = 4, 6
    color, depth, plane = np.zeros((h, w, 3), dtype=np.float32), np.zeros((h, w), dtype=np.float32), np.zeros((3, h, w), dtype=np.float32)
    with pytest.raises(ValueError, match="return_confidence"):
        ra.temporal_accumulate(color, color, depth, plane, plane, demodulate=False, return_confidence=True)
    with pytest.raises(ValueError, match="clip"):
        ra.temporal_accumulate(color, color, depth, plane, plane, demodulate=False, clip=dict(window=3))
    vp = ra.Viewport(16, 16, seed=1)
    with pytest.raises(ValueError, match="temporal=True"):
        vp.denoise(ra.RtPassParams(), clip=True)
    with pytest.raises(ValueError, match="return_confidence"):
        vp.denoise(ra.RtPassParams(), temporal=True, return_confidence=True)
    with pytest.raises(RuntimeError, match="set_renderer"):
        vp.denoise(ra.RtPassParams(), temporal=True, clip=True)
