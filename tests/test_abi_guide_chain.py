"""The C ABI of guide chains (include/rtgpu.h: rtgpu_render_aovs_chain, rtgpu_set_guide_chain), the part that needs no GPU: the symbols, the chain block's
layout, the plane ids, the checks that come before any device work, and the wrapper's own refusals.  The device side: tests/test_gpu_guide_chain.py."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("rtgpu_render_aovs_chain", "rtgpu_render_aovs_chain_async", "rtgpu_set_guide_chain")
INVALID_ARGUMENT = -1


def test_symbols_are_exported_and_the_abi_version_stays(built):
    import raytracer_amd as ra
    lib = ra.rtgpu_lib()
    text = open(os.path.join(ROOT, "include", "rtgpu.h")).read()
    for name in ENTRIES:
        assert hasattr(lib, name), name
        assert re.search(r"\bint %s\(" % name, text), name
    assert lib.rtgpu_abi_version() == 3   # added functions: no bump
    assert re.search(r"#define RTGPU_ABI_VERSION 3u\b", text)


def test_the_chain_block_is_16_bytes_and_mirrors_the_header(built):
    import raytracer_amd as ra
    assert C.sizeof(ra.RtAovChain) == 16
    text = open(os.path.join(ROOT, "include", "rtgpu.h")).read()
    body = re.search(r"typedef struct RtAovChain\s*\{(.*?)\} RtAovChain;", text, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = re.findall(r"uint32_t\s+(\w+)(?:\[(\d+)\])?;", body)
    assert [name for name, _ in fields] == [name for name, _ in ra.RtAovChain._fields_] == ["maxChain", "flags", "_pad"]
    assert ra.RtAovChain.maxChain.offset == 0 and ra.RtAovChain.flags.offset == 4 and ra.RtAovChain._pad.offset == 8 and fields[2][1] == "2"
    assert ra.AOV_CHAIN_MAX == 16 and re.search(r"#define RT_AOV_CHAIN_MAX 16u\b", text)


def test_the_chain_planes_lie_behind_the_first_hit_planes(built):
    import raytracer_amd as ra
    assert list(ra.AOV_PLANES)[-1] == "triangle_tests_passed" and len(ra.AOV_PLANES) == 19   # AOV_PLANES stays as it is
    n = len(ra.AOV_PLANES)
    assert list(ra.AOV_CHAIN_PLANES.items()) == [("chain_length", (n, 1, np.uint32)), ("chain_distance", (n + 1, 1, np.float32)), ("chain_throughput", (n + 2, 3, np.float32))]
    text = open(os.path.join(ROOT, "include", "rtgpu.h")).read()
    body = re.search(r"typedef enum RtAovChainPlane\s*\{(.*?)\} RtAovChainPlane;", text, flags=re.S).group(1)
    names = re.findall(r"\b(RT_AOV_CHAIN_\w+)\b", re.sub(r"/\*.*?\*/", "", body, flags=re.S))
    assert names == ["RT_AOV_CHAIN_LENGTH", "RT_AOV_CHAIN_DISTANCE", "RT_AOV_CHAIN_THROUGHPUT", "RT_AOV_CHAIN_NUM_PLANES"]
    assert re.search(r"RT_AOV_CHAIN_LENGTH\s*=\s*RT_AOV_NUM_PLANES\b", body)


def test_a_null_context_is_refused_before_anything_else(built):
    import raytracer_amd as ra
    lib = ra.rtgpu_lib()
    p, chain = ra.RtPassParams(), ra.RtAovChain(2, 0)
    ids = (C.c_uint32 * 1)(0)
    a = np.zeros(64, dtype=np.float32)
    ptrs = (C.c_void_p * 1)(a.ctypes.data)
    assert lib.rtgpu_render_aovs_chain(None, C.byref(p), C.byref(chain), ids, 1, ptrs) == INVALID_ARGUMENT and b"NULL" in lib.rtgpu_last_error()
    assert lib.rtgpu_render_aovs_chain_async(None, C.byref(p), C.byref(chain), ids, 1, ptrs, None) == INVALID_ARGUMENT
    assert lib.rtgpu_render_aovs_chain(None, None, None, None, 0, None) == INVALID_ARGUMENT   # even an empty call needs a context
    assert lib.rtgpu_set_guide_chain(None, C.byref(chain)) == INVALID_ARGUMENT and lib.rtgpu_set_guide_chain(None, None) == INVALID_ARGUMENT


def test_wrapper_refusals(built):
    import raytracer_amd as ra
    vp = ra.Viewport(16, 16, seed=1)
    with pytest.raises(ValueError, match="chain=N"):      # a chain plane without a chain
        vp.render_aovs(ra.RtPassParams(), ("depth", "chain_length"))
    with pytest.raises(ValueError, match="unknown AOV plane"):
        vp.render_aovs(ra.RtPassParams(), ("chain_width",), chain=2)
    with pytest.raises(TypeError, match="next_pass_params"):
        vp.render_aovs(None, ("depth",), chain=2)
    with pytest.raises(RuntimeError, match="set_renderer"):   # well-formed arguments get as far as the missing renderer
        vp.render_aovs(ra.RtPassParams(), ("depth", "chain_length"), chain=2)
    with pytest.raises(RuntimeError, match="set_renderer"):
        vp.set_guide_chain(2)
