"""The C ABI of moving objects (include/rtgpu.h: rtgpu_update_objects, rtgpu_get_update_info), the part that needs no GPU: the symbols, the two
structs' layouts against the header, and the checks that come before any device work.  The device side: tests/test_gpu_update.py."""
import ctypes as C
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("rtgpu_update_objects", "rtgpu_get_update_info")
HOST_ENTRIES = ("rth_scene_object_count", "rth_scene_object_set_transform", "rth_scene_update", "rth_scene_update_desc", "rth_viewport_update_scene")
INVALID_ARGUMENT = -1


def _header():
    return open(os.path.join(ROOT, "include", "rtgpu.h")).read()


def test_symbols_are_exported_and_the_abi_version_stays(built):
    import raytracer_amd as ra
    lib, host = ra.rtgpu_lib(), ra.host_lib()
    for name in ENTRIES:
        assert hasattr(lib, name), name
        assert re.search(r"\bint %s\(" % name, _header()), name
    for name in HOST_ENTRIES:
        assert hasattr(host, name), name
    assert lib.rtgpu_abi_version() == 3   # added functions, no struct changed: no bump
    assert int(re.search(r"#define RTGPU_ABI_VERSION (\d+)u", _header()).group(1)) == 3


def test_scene_update_mirrors_the_header(built):
    import raytracer_amd as ra
    body = re.search(r"typedef struct RtSceneUpdate\s*\{(.*?)\} RtSceneUpdate;", _header(), flags=re.S).group(1)
    words = [n.strip() for n in re.search(r"^\s*uint32_t\s+([\w, ]+);", body, flags=re.M).group(1).split(",")]
    pointers = re.findall(r"^\s*const\s+(\w+)\s*\*\s*(\w+);", body, flags=re.M)
    names = words + [name for _, name in pointers]
    assert names == [name for name, _ in ra.RtSceneUpdate._fields_] == ["abiVersion", "numObjects", "numTopNodes", "numLights", "topNodes", "objects", "previousIndex", "lights"]
    assert [t for t, _ in pointers] == ["RtNode", "RtObject", "uint32_t", "RtLight"]
    offset = 0
    for name in words:
        assert getattr(ra.RtSceneUpdate, name).offset == offset, name
        offset += 4
    for _, name in pointers:
        assert getattr(ra.RtSceneUpdate, name).offset == offset, name
        offset += C.sizeof(C.c_void_p)
    assert C.sizeof(ra.RtSceneUpdate) == offset == 48
    # the records an update is made of keep their sizes (the contract compares them bytewise behind the two matrices)
    assert (C.sizeof(ra.RtNode), C.sizeof(ra.RtObject), C.sizeof(ra.RtLight)) == (32, 192, 208)
    assert ra.RtObject.objectKind.offset == ra.RtLight.color.offset == 128


def test_update_info_mirrors_the_header(built):
    import raytracer_amd as ra
    body = re.search(r"typedef struct RtUpdateInfo\s*\{(.*?)\} RtUpdateInfo;", _header(), flags=re.S).group(1)
    assert re.sub(r"\s+", " ", body).strip() == "uint64_t bytesUploaded; uint32_t numUpdates, topDepth; uint32_t walk; uint32_t _pad[3];"
    assert [name for name, _ in ra.RtUpdateInfo._fields_] == ["bytesUploaded", "numUpdates", "topDepth", "walk", "_pad"]
    assert [getattr(ra.RtUpdateInfo, n).offset for n in ("bytesUploaded", "numUpdates", "topDepth", "walk", "_pad")] == [0, 8, 12, 16, 20]
    assert C.sizeof(ra.RtUpdateInfo) == 32
    text = _header()
    assert [int(re.search(r"#define RTGPU_WALK_%s\s+(\d)u" % k, text).group(1)) for k in ("BINARY", "WIDE", "WIDE2")] == [0, 1, 2]   # update_info()'s names


def test_object_motion_mirrors_the_header(built):
    import numpy as np
    import raytracer_amd as ra
    body = re.search(r"typedef struct RtObjectMotion\s*\{(.*?)\} RtObjectMotion;", _header(), flags=re.S).group(1)
    assert re.sub(r"\s+", " ", body).strip() == "float m[16]; uint32_t prevId; uint32_t moved; uint32_t _pad[2];"
    assert [name for name, _ in ra.RtObjectMotion._fields_] == ["m", "prevId", "moved", "_pad"]
    assert [getattr(ra.RtObjectMotion, n).offset for n in ("m", "prevId", "moved", "_pad")] == [0, 64, 68, 72] and C.sizeof(ra.RtObjectMotion) == 80
    for name in ("rtgpu_temporal_accumulate_moving", "rtgpu_temporal_accumulate_moving_async"):
        assert hasattr(ra.rtgpu_lib(), name) and re.search(r"\bint %s\(" % name, _header()), name
    # the wrapper's table is that record, word for word
    m = np.arange(32, dtype=np.float32).reshape(2, 4, 4)
    table = ra.object_motion_table((m, [5, 6], [0, 3]))
    assert table.shape == (2, 20) and table.dtype == np.uint32
    record = ra.RtObjectMotion.from_buffer_copy(table[1].tobytes())
    assert list(record.m) == list(range(16, 32)) and (record.prevId, record.moved, list(record._pad)) == (6, 1, [0, 0])
    # the moving entries refuse a NULL context like the others
    t = ra.temporal_params()
    ptr = m.ctypes.data_as(C.c_void_p)
    args = (None, C.byref(t), C.c_uint32(2), C.c_uint32(2)) + (ptr,) * 18 + (table.ctypes.data_as(C.c_void_p), C.c_uint32(2))
    assert ra.rtgpu_lib().rtgpu_temporal_accumulate_moving(*args) == INVALID_ARGUMENT
    assert ra.rtgpu_lib().rtgpu_temporal_accumulate_moving_async(*(args + (None,))) == INVALID_ARGUMENT


def test_null_arguments_are_refused_before_anything_else(built):
    import raytracer_amd as ra
    lib = ra.rtgpu_lib()
    u, info = ra.RtSceneUpdate(), ra.RtUpdateInfo()
    assert lib.rtgpu_update_objects(None, C.byref(u)) == INVALID_ARGUMENT and b"NULL" in lib.rtgpu_last_error()
    assert lib.rtgpu_update_objects(None, None) == INVALID_ARGUMENT
    assert lib.rtgpu_get_update_info(None, C.byref(info)) == INVALID_ARGUMENT and b"NULL" in lib.rtgpu_last_error()
    with pytest.raises(RuntimeError):
        ra.update_info(None)


def test_wrapper_refusals_without_a_renderer(built):
    import raytracer_amd as ra
    vp = ra.Viewport(16, 16, seed=1)
    with pytest.raises(RuntimeError, match="UpdateScene"):
        vp.update_scene()
    s = ra.Scene()
    with pytest.raises(IndexError):
        s.set_object_transform(0, ra.transform_from_euler())
    with pytest.raises(RuntimeError, match="build"):
        s.update()
