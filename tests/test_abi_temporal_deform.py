"""The C ABI of temporal accumulation that follows deforming meshes (include/rtgpu.h: rtgpu_temporal_accumulate_deform, rtgpu_set_deform_tracking), the part
that needs no GPU: the symbols, the block's layout, what must not have changed beside them, the checks that come before any device work, and the wrappers' own
refusals.  The device side, with the refusals that need a context: tests/test_gpu_temporal_deform.py."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("rtgpu_temporal_accumulate_deform", "rtgpu_temporal_accumulate_deform_async", "rtgpu_set_deform_tracking")
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


def test_the_deform_block_is_32_bytes_and_the_motion_record_keeps_its_80(built):
    import raytracer_amd as ra
    text = header()
    assert C.sizeof(ra.RtTemporalDeform) == 32 and C.sizeof(ra.RtObjectMotion) == 80
    assert re.search(r"#define RT_MOTION_DEFORMED 2u\b", text) and ra.RT_MOTION_DEFORMED == 2
    body = re.search(r"typedef struct RtTemporalDeform\s*\{(.*?)\} RtTemporalDeform;", text, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    assert re.findall(r"const\s+(float|uint32_t|RtTriangle)\*\s+(\w+);", body) == [("uint32_t", "subObjectId"), ("float", "barycentrics"), ("RtTriangle", "prevTriangles")]
    assert re.search(r"uint32_t\s+numPrevTriangles,\s*_pad;", body)
    assert [name for name, _ in ra.RtTemporalDeform._fields_] == ["subObjectId", "barycentrics", "prevTriangles", "numPrevTriangles", "_pad"]
    assert [getattr(ra.RtTemporalDeform, name).offset for name, _ in ra.RtTemporalDeform._fields_] == [0, 8, 16, 24, 28]
    # the motion record: the same five fields at the same offsets
    assert re.search(r"typedef struct RtObjectMotion \{ float m\[16\]; uint32_t prevId; uint32_t moved; uint32_t _pad\[2\]; \} RtObjectMotion;", text)
    assert [getattr(ra.RtObjectMotion, name).offset for name in ("m", "prevId", "moved", "_pad")] == [0, 64, 68, 72]
    assert ra.DEFORM_KEYS == ("sub_object_id", "barycentrics", "prev_triangles", "first_triangle", "num_triangles")
    assert ra.HISTORY_KEYS == ("a", "b", "length", "depth", "normal", "position", "object_id")


def test_the_table_of_a_deform_call_carries_moved_and_the_triangle_ranges(built):
    import raytracer_amd as ra
    motion = (np.tile(np.eye(4, dtype=np.float32), (3, 1, 1)), [2, 1, 0], [0, 1, 2])
    plain = ra.object_motion_table((motion[0], motion[1], [0, 5, 2]))
    assert plain[:, 17].tolist() == [0, 1, 1] and not plain[:, 18:].any()      # without deform: moved is a flag, as ever
    table = ra.object_motion_table(motion, dict(first_triangle=[0, 0, 7], num_triangles=[0, 0, 512]))
    assert table.shape == (3, 20) and table[:, 16].tolist() == [2, 1, 0] and table[:, 17].tolist() == [0, 1, 2] and table[:, 18].tolist() == [0, 0, 7] and table[:, 19].tolist() == [0, 0, 512]
    with pytest.raises(ValueError, match="one value per record"):
        ra.object_motion_table(motion, dict(first_triangle=[0, 7], num_triangles=[0, 0, 512]))


def test_a_null_context_is_refused_before_anything_else(built):
    import raytracer_amd as ra
    lib = ra.rtgpu_lib()
    a = np.zeros(64, dtype=np.float32)
    t = ra.temporal_params()
    table = ra.object_motion_table((np.eye(4, dtype=np.float32)[None], [0], [2]), dict(first_triangle=[0], num_triangles=[1]))
    block = ra.RtTemporalDeform(a.ctypes.data, a.ctypes.data, a.ctypes.data, 1, 0)
    pure = [None, C.byref(t), C.c_uint32(1), C.c_uint32(1)] + [C.c_void_p(a.ctypes.data)] * 5 + [None] * 9 + [C.c_void_p(a.ctypes.data)] * 3 + [
        None, C.c_void_p(table.ctypes.data), C.c_uint32(1), None, None, C.byref(block)]
    assert lib.rtgpu_temporal_accumulate_deform(*pure) == INVALID_ARGUMENT and b"NULL context" in lib.rtgpu_last_error()
    assert lib.rtgpu_temporal_accumulate_deform_async(*(pure + [None])) == INVALID_ARGUMENT and b"NULL context" in lib.rtgpu_last_error()
    assert lib.rtgpu_set_deform_tracking(None, 1) == INVALID_ARGUMENT and b"NULL context" in lib.rtgpu_last_error()


def test_wrapper_refusals(built):
    import raytracer_amd as ra
    vp = ra.Viewport(16, 16, seed=1)
    vp.track_deformation()            # before the device context exists: remembered, not an error
    assert vp._track_deformation is True
    vp.track_deformation(False)
    assert vp._track_deformation is False
    h, w = 4, 6
    image, plane3, plane1 = np.zeros((h, w, 3), dtype=np.float32), np.zeros((3, h, w), dtype=np.float32), np.ones((h, w), dtype=np.float32)
    ids = np.zeros((h, w), dtype=np.uint32)
    motion = (np.eye(4, dtype=np.float32)[None], [0], [2])
    deform = dict(sub_object_id=ids, barycentrics=np.zeros((2, h, w), dtype=np.float32), prev_triangles=np.zeros((1, 9), dtype=np.float32), first_triangle=[0], num_triangles=[1])
    frame = dict(color=image, color_half=image, depth=plane1, normal=plane3, position=plane3, object_id=ids, demodulate=False)
    with pytest.raises(ValueError, match="sub_object_id"):
        ra.temporal_accumulate(deform=dict(sub_object_id=ids), object_motion=motion, **frame)
    with pytest.raises(ValueError, match="goes with object_motion"):
        ra.temporal_accumulate(deform=deform, **frame)
    chain = dict(virtual_position=plane3, chain_length=ids, chain_distance=plane1)
    with pytest.raises(ValueError, match="without chain"):
        ra.temporal_accumulate(deform=deform, object_motion=motion, chain=chain, **frame)
    with pytest.raises(ValueError, match="barycentrics must be a float32"):
        ra.temporal_accumulate(deform=dict(deform, barycentrics=plane3), object_motion=motion, **frame)
    with pytest.raises(ValueError, match="sub_object_id must be a uint32"):
        ra.temporal_accumulate(deform=dict(deform, sub_object_id=plane1), object_motion=motion, **frame)
