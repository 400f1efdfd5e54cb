"""The C ABI of the virtual position and of temporal accumulation over chain guides (include/rtgpu.h: rtgpu_render_aovs_virtual, rtgpu_temporal_accumulate_chain,
rtgpu_denoise_temporal_chain), the part that needs no GPU: the symbols, the chain block's layout, the plane ids, what must not have changed beside them, the
checks that come before any device work, and the wrappers' own refusals.  The device side: tests/test_gpu_virtual_plane.py, tests/test_gpu_temporal_chain.py."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("rtgpu_render_aovs_virtual", "rtgpu_render_aovs_virtual_async", "rtgpu_temporal_accumulate_chain", "rtgpu_temporal_accumulate_chain_async",
           "rtgpu_denoise_temporal_chain", "rtgpu_denoise_temporal_chain_async")
INVALID_ARGUMENT = -1


def header():
    return open(os.path.join(ROOT, "include", "rtgpu.h")).read()


def test_symbols_are_exported_and_the_abi_version_stays(built):
    import raytracer_amd as ra
    lib = ra.rtgpu_lib()
    text = header()
    for name in ENTRIES:
        assert hasattr(lib, name), name
        assert re.search(r"\bint %s\(" % name, text), name
    assert lib.rtgpu_abi_version() == 3   # added functions: no bump
    assert re.search(r"#define RTGPU_ABI_VERSION 3u\b", text)


def test_the_temporal_chain_block_is_32_bytes_and_mirrors_the_header(built):
    import raytracer_amd as ra
    assert C.sizeof(ra.RtTemporalChain) == 32
    body = re.search(r"typedef struct RtTemporalChain\s*\{(.*?)\} RtTemporalChain;", header(), flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = re.findall(r"const\s+(float|uint32_t)\*\s+(\w+);", body)
    assert fields == [("float", "virtualPosition"), ("uint32_t", "chainLength"), ("float", "chainDistance"), ("uint32_t", "prevChainLength")]
    assert [name for name, _ in ra.RtTemporalChain._fields_] == [name for _, name in fields]
    assert [getattr(ra.RtTemporalChain, name).offset for _, name in fields] == [0, 8, 16, 24]
    assert ra.CHAIN_KEYS == ("virtual_position", "chain_length", "chain_distance")


def test_the_virtual_plane_lies_behind_the_chain_planes_which_stay(built):
    import raytracer_amd as ra
    text = header()
    body = re.search(r"typedef enum RtAovVirtualPlane\s*\{(.*?)\} RtAovVirtualPlane;", text, flags=re.S).group(1)
    names = re.findall(r"\b(RT_AOV_VIRTUAL_\w+)\b", re.sub(r"/\*.*?\*/", "", body, flags=re.S))
    assert names == ["RT_AOV_VIRTUAL_POSITION", "RT_AOV_VIRTUAL_NUM_PLANES"]
    assert re.search(r"RT_AOV_VIRTUAL_POSITION\s*=\s*RT_AOV_CHAIN_NUM_PLANES\b", body)
    n = len(ra.AOV_PLANES)
    assert n == 19
    assert list(ra.AOV_VIRTUAL_PLANES.items()) == [("virtual_position", (n + len(ra.AOV_CHAIN_PLANES), 3, np.float32))] == [("virtual_position", (22, 3, np.float32))]
    # what stays: the chain enum's four enumerators, the chain table's three entries, the history's keys
    chain = re.search(r"typedef enum RtAovChainPlane\s*\{(.*?)\} RtAovChainPlane;", text, flags=re.S).group(1)
    assert re.findall(r"\b(RT_AOV_\w+)\b", re.sub(r"/\*.*?\*/", "", chain, flags=re.S)) == [
        "RT_AOV_CHAIN_LENGTH", "RT_AOV_NUM_PLANES", "RT_AOV_CHAIN_DISTANCE", "RT_AOV_CHAIN_THROUGHPUT", "RT_AOV_CHAIN_NUM_PLANES"]
    assert list(ra.AOV_CHAIN_PLANES.items()) == [("chain_length", (n, 1, np.uint32)), ("chain_distance", (n + 1, 1, np.float32)), ("chain_throughput", (n + 2, 3, np.float32))]
    assert ra.HISTORY_KEYS == ("a", "b", "length", "depth", "normal", "position", "object_id")


def test_a_null_context_is_refused_before_anything_else(built):
    import raytracer_amd as ra
    lib = ra.rtgpu_lib()
    p, chain = ra.RtPassParams(), ra.RtAovChain(2, 0)
    ids = (C.c_uint32 * 1)(22)
    a = np.zeros(64, dtype=np.float32)
    ptrs = (C.c_void_p * 1)(a.ctypes.data)
    assert lib.rtgpu_render_aovs_virtual(None, C.byref(p), C.byref(chain), ids, 1, ptrs) == INVALID_ARGUMENT and b"NULL" in lib.rtgpu_last_error()
    assert lib.rtgpu_render_aovs_virtual_async(None, C.byref(p), C.byref(chain), ids, 1, ptrs, None) == INVALID_ARGUMENT
    assert lib.rtgpu_render_aovs_virtual(None, None, None, None, 0, None) == INVALID_ARGUMENT   # even an empty call needs a context
    t = ra.temporal_params()
    block = ra.RtTemporalChain(a.ctypes.data, a.ctypes.data, a.ctypes.data, None)
    pure = [None, C.byref(t), C.c_uint32(1), C.c_uint32(1)] + [C.c_void_p(a.ctypes.data)] * 5 + [None] * 9 + [C.c_void_p(a.ctypes.data)] * 3 + [None, None, C.c_uint32(0), None, None,
                                                                                                                                        C.byref(block)]
    assert lib.rtgpu_temporal_accumulate_chain(*pure) == INVALID_ARGUMENT and b"NULL context" in lib.rtgpu_last_error()
    assert lib.rtgpu_temporal_accumulate_chain_async(*(pure + [None])) == INVALID_ARGUMENT
    frame = (None, C.byref(t), None, C.byref(p), C.byref(chain), C.c_void_p(a.ctypes.data), None, None, None)
    assert lib.rtgpu_denoise_temporal_chain(*frame) == INVALID_ARGUMENT and b"NULL context" in lib.rtgpu_last_error()
    assert lib.rtgpu_denoise_temporal_chain_async(*(frame + (None,))) == INVALID_ARGUMENT


def test_wrapper_refusals(built):
    import raytracer_amd as ra
    vp = ra.Viewport(16, 16, seed=1)
    with pytest.raises(ValueError, match="chain=N"):      # the virtual plane without a chain: what a chain plane raises
        vp.render_aovs(ra.RtPassParams(), ("depth", "virtual_position"))
    with pytest.raises(RuntimeError, match="set_renderer"):   # well-formed arguments get as far as the missing renderer
        vp.render_aovs(ra.RtPassParams(), ("depth", "virtual_position"), chain=2)
    with pytest.raises(ValueError, match="temporal=True"):
        vp.denoise(ra.RtPassParams(), chain=2)
    with pytest.raises(ValueError, match="temporal=True"):
        vp.denoise(ra.RtPassParams(), variance=True, chain=0)
    with pytest.raises(RuntimeError, match="set_renderer"):
        vp.denoise(ra.RtPassParams(), temporal=True, chain=2)
    h, w = 4, 6
    image, plane3, plane1 = np.zeros((h, w, 3), dtype=np.float32), np.zeros((3, h, w), dtype=np.float32), np.ones((h, w), dtype=np.float32)
    k = np.zeros((h, w), dtype=np.uint32)
    chain = dict(virtual_position=plane3, chain_length=k, chain_distance=plane1)
    frame = dict(color=image, color_half=image, depth=plane1, normal=plane3, position=plane3, demodulate=False)
    with pytest.raises(ValueError, match="virtual_position"):
        ra.temporal_accumulate(chain=dict(virtual_position=plane3, chain_length=k), **frame)
    with pytest.raises(ValueError, match="virtual_position"):
        ra.temporal_accumulate(chain=plane3, **frame)
    plain = dict(a=image, b=image, length=plane1, depth=plane1, normal=plane3, position=plane3, object_id=None)   # a history of the calls without a chain
    with pytest.raises(ValueError, match="chain_length"):
        ra.temporal_accumulate(chain=chain, history=plain, prev_world_to_screen=np.eye(4), **frame)
    with pytest.raises(ValueError, match="chain_length must be a uint32"):
        ra.temporal_accumulate(chain=dict(chain, chain_length=plane1), **frame)
    with pytest.raises(ValueError, match="virtual_position must be a float32"):
        ra.temporal_accumulate(chain=dict(chain, virtual_position=plane1), **frame)
