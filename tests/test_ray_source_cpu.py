"""The ray source (include/rtgpu.h: rtgpu_set_ray_source, rtgpu_read_camera_rays), the part that needs no GPU: the symbols and the entry's layout, the checks
that come before any device work, the wrappers' own refusals, and the NumPy builders of raytracer_amd/rays.py.  The device side:
tests/test_gpu_ray_source.py."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("rtgpu_set_ray_source", "rtgpu_set_ray_source_device", "rtgpu_get_ray_source", "rtgpu_read_camera_rays", "rtgpu_read_camera_rays_async")
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
        assert getattr(lib, name).argtypes is not None, name   # the ctypes mirror declares it
    assert lib.rtgpu_abi_version() == 3   # added functions: no bump
    assert int(re.search(r"#define RTGPU_ABI_VERSION (\d+)u", text).group(1)) == 3


def test_the_entry_is_32_bytes_and_has_the_query_rays_layout(built):
    import raytracer_amd as ra
    assert C.sizeof(ra.RtPrimaryRay) == 32 == C.sizeof(ra.RtQueryRay)
    body = re.search(r"typedef struct RtPrimaryRay\s*\{(.*?)\} RtPrimaryRay;", header(), flags=re.S).group(1)
    fields = re.findall(r"float\s+(\w+)(\[\d+\])?;", body)
    assert [name for name, _ in fields] == [name for name, _ in ra.RtPrimaryRay._fields_] == ["origin", "_pad0", "direction", "_pad1"]
    offset = 0
    for (name, array), (_, mirror) in zip(fields, ra.RtPrimaryRay._fields_):
        assert getattr(ra.RtPrimaryRay, name).offset == offset, name
        assert C.sizeof(mirror) == 4 * (int(array[1:-1]) if array else 1), name
        offset += C.sizeof(mirror)
    assert offset == 32
    # one buffer serves this call and rtgpu_trace_rays
    assert ra.RtPrimaryRay.origin.offset == ra.RtQueryRay.origin.offset == 0 and ra.RtPrimaryRay.direction.offset == ra.RtQueryRay.direction.offset == 16


def test_a_null_context_is_refused_before_anything_else(built):
    import raytracer_amd as ra
    lib = ra.rtgpu_lib()
    a = np.zeros(64, dtype=np.float32)
    ptr, n, pp = a.ctypes.data_as(C.c_void_p), C.c_uint64(0), ra.RtPassParams()
    assert lib.rtgpu_set_ray_source(None, ptr, C.c_uint64(8)) == INVALID_ARGUMENT and b"NULL" in lib.rtgpu_last_error()
    assert lib.rtgpu_set_ray_source_device(None, ptr, C.c_uint64(8), None) == INVALID_ARGUMENT
    assert lib.rtgpu_get_ray_source(None, C.byref(n)) == INVALID_ARGUMENT
    assert lib.rtgpu_read_camera_rays(None, C.byref(pp), ptr) == INVALID_ARGUMENT
    assert lib.rtgpu_read_camera_rays_async(None, C.byref(pp), ptr, None) == INVALID_ARGUMENT


def test_wrapper_refusals(built):
    import raytracer_amd as ra
    vp = ra.Viewport(6, 4, seed=1)
    assert vp.ray_source() is False
    with pytest.raises(RuntimeError, match="set_renderer"):
        vp.set_ray_source(np.zeros((4, 6, 8), dtype=np.float32))
    with pytest.raises(RuntimeError, match="set_renderer"):
        vp.camera_rays(ra.RtPassParams())
    with pytest.raises(TypeError, match="next_pass_params"):
        vp.camera_rays(None)


# ---- the builders ------------------------------------------------------------------------------------------------------------------------------------
def transform(right=(1, 0, 0), up=(0, 1, 0), forward=(0, 0, 1), position=(0, 0, 0)):
    m = np.zeros((4, 4), dtype=np.float32)
    m[0, :3], m[1, :3], m[2, :3], m[3, :3] = right, up, forward, position
    m[3, 3] = 1.0
    return m


TILTED = transform(right=(0.6, 0.0, -0.8), up=(0.0, 1.0, 0.0), forward=(0.8, 0.0, 0.6), position=(1.5, -2.0, 0.25))


def sound(origins, directions, shape):
    assert origins.dtype == directions.dtype == np.float32
    assert origins.shape == directions.shape == shape
    assert np.isfinite(origins).all() and np.isfinite(directions).all()
    assert (np.einsum("...k,...k->...", directions, directions) > 0.0).all()


def angle(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.arccos(np.clip(np.dot(a, b) / np.sqrt(np.dot(a, a) * np.dot(b, b)), -1.0, 1.0)))


def test_orthographic_rays_are_parallel_and_evenly_spaced():
    from raytracer_amd import rays
    w, h, half = 37, 23, 2.5
    o, d = rays.orthographic(w, h, TILTED, half)
    sound(o, d, (h, w, 3))
    assert (d == d[0, 0]).all() and angle(d[0, 0], TILTED[2, :3]) < 1e-6
    step = 2.0 * half / w
    dx, dy = o[:, 1:] - o[:, :-1], o[1:] - o[:-1]
    assert np.allclose(np.linalg.norm(dx, axis=-1), step, atol=1e-5) and np.allclose(np.linalg.norm(dy, axis=-1), step, atol=1e-5)
    assert np.allclose(dx, step * TILTED[0, :3], atol=1e-5)      # columns go right
    assert np.allclose(dy, -step * TILTED[1, :3], atol=1e-5)     # rows go down: row 0 is the top
    assert np.allclose(o[h // 2, w // 2], TILTED[3, :3], atol=1e-5)   # centred on the transform's position (odd sizes: a pixel's centre)
    # a sample offset moves the sample by pixels, x right and y up
    o2, _ = rays.orthographic(w, h, TILTED, half, sample_offset=(0.25, -0.5))
    assert np.allclose(o2 - o, step * (0.25 * TILTED[0, :3] - 0.5 * TILTED[1, :3]), atol=1e-5)


def test_panorama_covers_the_sphere_once():
    from raytracer_amd import rays
    w, h = 73, 37
    o, d = rays.panorama(w, h, TILTED)
    sound(o, d, (h, w, 3))
    right, up, forward = TILTED[0, :3].astype(np.float64), TILTED[1, :3].astype(np.float64), TILTED[2, :3].astype(np.float64)
    assert (o == TILTED[3, :3]).all()
    assert angle(d[h // 2, w // 2], forward) < 1e-6
    # rows sweep from up to down: the elevation falls monotonically from just below +pi/2 to just above -pi/2
    elevation = np.arcsin(np.clip(d.astype(np.float64) @ up, -1.0, 1.0))
    assert (np.abs(elevation - elevation[:, :1]) < 1e-6).all()
    assert (np.diff(elevation[:, 0]) < 0.0).all()
    assert abs(elevation[0, 0] - (np.pi / 2 - np.pi / (2 * h))) < 1e-6 and abs(elevation[-1, 0] + (np.pi / 2 - np.pi / (2 * h))) < 1e-6
    # columns go once around, turning right from the centre
    row = d[h // 2].astype(np.float64)
    azimuth = np.arctan2(row @ right, row @ forward)
    assert (np.diff(azimuth) > 0.0).all()
    assert np.allclose(np.diff(azimuth), 2 * np.pi / w, atol=1e-5)
    assert abs(azimuth[0] + np.pi - np.pi / w) < 1e-5 and abs(azimuth[-1] - np.pi + np.pi / w) < 1e-5


def test_fisheye_reaches_half_the_fov_on_the_image_circle():
    from raytracer_amd import rays
    n, fov = 65, np.deg2rad(200.0)
    forward = TILTED[2, :3]
    o, d = rays.fisheye(n, n, TILTED, fov)
    sound(o, d, (n, n, 3))
    assert angle(d[n // 2, n // 2], forward) < 1e-6                        # the centre pixel: the axis
    theta = np.array([angle(d[n // 2, x], forward) for x in range(n)])
    assert np.allclose(theta, np.abs(2.0 * (np.arange(n) + 0.5) / n - 1.0) * fov / 2, atol=1e-5)   # equidistant: the angle is linear in the radius
    # the sample of the last column moved half a pixel right lies ON the image circle: fov / 2 with the axis
    _, edge = rays.fisheye(n, n, TILTED, fov, sample_offset=(0.5, 0.0))
    assert abs(angle(edge[n // 2, n - 1], forward) - fov / 2) < 1e-5
    # outside the circle the axis ray repeats
    for y, x in ((0, 0), (0, n - 1), (n - 1, 0), (n - 1, n - 1)):
        assert angle(d[y, x], forward) < 1e-6
    # a wide picture: the circle is inscribed in the shorter side
    # (column c of the middle row sits at x = 2 * ((c + 0.5) / n - 1) radii from the centre: c = 97 is on the circle, the first column far outside)
    _, wide = rays.fisheye(2 * n, n, TILTED, fov)
    assert abs(angle(wide[n // 2, 97], forward) - fov / 2) < 1e-5 and angle(wide[n // 2, 98], forward) < 1e-6 and angle(wide[n // 2, 0], forward) < 1e-6


def test_hemisphere_probe_leaves_the_surface():
    from raytracer_amd import rays
    rng = np.random.default_rng(5)
    points = rng.uniform(-3, 3, (9, 3))
    normals = rng.normal(size=(9, 3))
    normals[0], normals[1], normals[2] = (0, 0, 1), (0, 0, -1), (0, -2, 0)
    n = 64
    o, d = rays.hemisphere_probe(points, normals, n)
    sound(o, d, (9, n, 3))
    unit = normals / np.linalg.norm(normals, axis=1, keepdims=True)
    cosine = np.einsum("pjk,pk->pj", d.astype(np.float64), unit)
    assert (cosine > 0.0).all()
    assert np.allclose(o, (points + 1e-3 * unit)[:, None, :], atol=1e-6)    # one point per row, lifted off the surface
    assert abs(cosine.mean() - 2.0 / 3.0) < 0.02                             # cosine-distributed: E[cos] = 2 / 3
    o2, d2 = rays.hemisphere_probe(points, normals, n, sample_offset=(0.37, 0.61), offset=0.0)
    assert np.allclose(o2, points[:, None, :], atol=1e-6) and not np.allclose(d2, d)
    assert (np.einsum("pjk,pk->pj", d2.astype(np.float64), unit) > 0.0).all()


@pytest.mark.parametrize("size", [(1, 1), (70, 1), (37, 23)])
def test_every_builder_returns_sound_tables(size):
    from raytracer_amd import rays
    w, h = size
    for o, d in (rays.orthographic(w, h, TILTED, 1.0), rays.panorama(w, h, TILTED), rays.fisheye(w, h, TILTED, np.pi),
                 rays.orthographic(w, h, TILTED, 1.0, sample_offset=(0.3, -0.2)), rays.panorama(w, h, TILTED, sample_offset=(-0.5, 0.5)),
                 rays.fisheye(w, h, TILTED, 2 * np.pi, sample_offset=(0.5, 0.5))):
        sound(o, d, (h, w, 3))
    with pytest.raises(ValueError):
        rays.orthographic(w, h, TILTED, 0.0)
    with pytest.raises(ValueError):
        rays.fisheye(w, h, TILTED, 0.0)
    with pytest.raises(ValueError):
        rays.hemisphere_probe([[0, 0, 0]], [[0, 0, 0]], 4)
