"""The DEVICE functions at the edges of their domains: tests/golden/edges/*.kat (records the reference's own translation units computed from
explicit bit patterns: thresholds with both float neighbours, signed zeros, denormals, infinities, NaN; tests/golden/README.md) through the
C-ABI's KAT hook rtgpu_kat, under the comparison of tests/test_gpu_kat.py (kat_io.edge_mismatch): NaN matches NaN, everything else bit for
bit; the two unused direction lanes may differ in the sign of a zero; the lanes behind the reference's _mm_rsqrt_ps agree to 2^-11 where the
expected value is finite and in class (NaN, +inf, -inf) where it is not.  tests/test_oracle_kat_edges.py holds the CPU oracle to the same
files and checks, from the fixtures alone, that every threshold shows both of its outcomes."""
import ctypes as C
import os

import numpy as np
import pytest

import kat_io

pytestmark = pytest.mark.gpu

EDGE_FILES = kat_io.edge_files()


@pytest.fixture(scope="module")
def ctx(built):
    import raytracer_amd as ra
    lib = ra.rtgpu_lib()
    c = C.c_void_p()
    assert lib.rtgpu_create(0, C.byref(c)) == 0, lib.rtgpu_last_error()
    yield lib, c
    lib.rtgpu_destroy(c)


def device_kat(lib, c, func, inputs, out_stride):
    inputs = np.ascontiguousarray(inputs, dtype=np.float32)
    n, in_stride = inputs.shape
    out = np.zeros((n, out_stride), dtype=np.float32)
    r = lib.rtgpu_kat(c, C.c_uint32(func), inputs.ctypes.data_as(C.c_void_p), C.c_uint32(in_stride), out.ctypes.data_as(C.c_void_p),
                      C.c_uint32(out_stride), C.c_uint32(n))
    assert r == 0, lib.rtgpu_last_error()
    return out


def test_edge_directory_covers_every_interior_function():
    """A function added to the interior fixtures without edge vectors fails here."""
    interior = {kat_io.load_kat(f)[0]: f for f in sorted(os.listdir(kat_io.GOLDEN)) if f.endswith(".kat") and not f.startswith("host_")}
    edges = {kat_io.load_kat(os.path.join("edges", f))[0] for f in EDGE_FILES}
    assert len(interior) >= 39
    missing = sorted(name for func, name in interior.items() if func not in edges)
    assert not missing, "no edge vectors under tests/golden/edges for %s" % missing


@pytest.mark.parametrize("name", EDGE_FILES)
def test_device_function_matches_reference_at_the_edges(ctx, name):
    lib, c = ctx
    func, inputs, expected = kat_io.load_kat(os.path.join("edges", name))
    got = device_kat(lib, c, func, inputs, expected.shape[1])
    bad = kat_io.edge_mismatch(name, inputs, expected, got)
    assert not bad.any(), kat_io.describe_edge_mismatch(name, func, inputs, expected, got, bad)
