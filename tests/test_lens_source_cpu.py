"""The lens source (include/rtgpu.h: rtgpu_set_lens_source, rtgpu_read_lens_source_rays, rtgpu_read_camera_footprints), the part that needs no GPU: the
symbols and the entry's layout, the refusals that come before any device work, the float32 model of the jitter step (tests/lens_source_ref.py) on
hand-computed values, and raytracer_amd.rays.footprints.  The device side: tests/test_gpu_lens_source.py."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import lens_source_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("rtgpu_set_lens_source", "rtgpu_set_lens_source_device", "rtgpu_get_ray_source_kind", "rtgpu_read_lens_source_rays", "rtgpu_read_lens_source_rays_async",
           "rtgpu_read_camera_footprints", "rtgpu_read_camera_footprints_async")
INVALID_ARGUMENT = -1
F = np.float32


def header():
    return open(os.path.join(ROOT, "include", "rtgpu.h")).read()


def test_symbols_are_exported_and_the_abi_version_stays(built):
    import raytracer_amd as ra
    lib = ra.rtgpu_lib()
    text = header()
    for name in ENTRIES:
        assert hasattr(lib, name), name
        assert re.search(r"\bint %s\(" % name, text), name
        assert getattr(lib, name).argtypes is not None, name
    assert lib.rtgpu_abi_version() == 3   # added functions: no bump


def test_the_entry_is_128_bytes_eight_quads(built):
    import raytracer_amd as ra
    assert C.sizeof(ra.RtLensRay) == 128 and C.sizeof(ra.RtLensSourceParams) == 8
    body = re.search(r"typedef struct RtLensRay\s*\{(.*?)\} RtLensRay;", header(), flags=re.S).group(1)
    fields = re.findall(r"float\s+(\w+)(\[\d+\])?;", body)
    assert [name for name, _ in fields] == [name for name, _ in ra.RtLensRay._fields_]
    offset = 0
    for (name, array), (_, mirror) in zip(fields, ra.RtLensRay._fields_):
        assert getattr(ra.RtLensRay, name).offset == offset, name
        assert C.sizeof(mirror) == 4 * (int(array[1:-1]) if array else 1), name
        offset += C.sizeof(mirror)
    assert offset == 128
    quads = ("origin", "direction", "dOriginDsx", "dOriginDsy", "dDirectionDsx", "dDirectionDsy", "lensU", "lensV")
    assert [getattr(ra.RtLensRay, q).offset for q in quads] == [16 * k for k in range(8)]
    assert ra.RtLensRay.aperture.offset == 12 and ra.RtLensRay.focalDistance.offset == 28


def test_refusals_before_any_device_work(built):
    import raytracer_amd as ra
    lib = ra.rtgpu_lib()
    table = np.zeros((2, 2, 32), dtype=np.float32)
    ptr = table.ctypes.data_as(C.c_void_p)
    good = ra.RtLensSourceParams(0, 0)
    kind = C.c_uint32(9)
    assert lib.rtgpu_set_lens_source(None, ptr, C.c_uint64(4), C.byref(good)) == INVALID_ARGUMENT
    assert lib.rtgpu_set_lens_source_device(None, ptr, C.c_uint64(4), C.byref(good), None) == INVALID_ARGUMENT
    assert lib.rtgpu_get_ray_source_kind(None, C.byref(kind)) == INVALID_ARGUMENT
    p = ra.RtPassParams()
    assert lib.rtgpu_read_lens_source_rays(None, C.byref(p), ptr) == INVALID_ARGUMENT
    assert lib.rtgpu_read_camera_footprints(None, C.byref(p), ptr) == INVALID_ARGUMENT
    vp = ra.Viewport(4, 4)
    with pytest.raises(RuntimeError, match="renderer"):
        vp.set_lens_source(np.zeros((4, 4, 32), dtype=np.float32))
    assert vp.ray_source_kind() == 0


# ---- the model's jitter step on hand-computed values ---------------------------------------------------------------------------------------------------
def entry(origin, direction, dodx=(0, 0, 0), dody=(0, 0, 0), dddx=(0, 0, 0), dddy=(0, 0, 0)):
    t = np.zeros((1, 1, 32), dtype=np.float32)
    t[0, 0, 0:3], t[0, 0, 4:7], t[0, 0, 8:11], t[0, 0, 12:15], t[0, 0, 16:19], t[0, 0, 20:23] = origin, direction, dodx, dody, dddx, dddy
    t[0, 0, 7] = 1.0
    t[0, 0, 24], t[0, 0, 29] = 1.0, 1.0
    return t


def test_the_jitter_step_on_hand_computed_values():
    t = entry((1.0, 2.0, 3.0), (0.0, 0.0, 1.0), dodx=(0.5, 0.0, 0.0), dody=(0.0, 0.25, 0.0), dddx=(0.125, 0.0, 0.0), dddy=(0.0, -0.5, 0.0))
    o, d = ref.jitter(t, 2.0, -4.0)   # every product and sum is exact in float32
    assert o[0, 0].tolist() == [2.0, 1.0, 3.0] and d[0, 0].tolist() == [0.25, 2.0, 1.0]
    assert o.dtype == np.float32 and d.dtype == np.float32
    # each operation rounds on its own: 1 + 2^-24 * 1 rounds to 1 (ties to even) before 2^-24 * 1 is added again -- a fused or exact sum would give 1 + 2^-23
    tiny = float(2.0 ** -24)
    t = entry((1.0, 0.0, 0.0), (0.0, 0.0, 1.0), dodx=(1.0, 0.0, 0.0), dody=(1.0, 0.0, 0.0))
    o, _ = ref.jitter(t, tiny, tiny)
    assert o[0, 0, 0] == F(1.0)
    # the product rounds before the sum: (1 + 2^-12)^2 = 1 + 2^-11 + 2^-24 rounds to 1 + 2^-11; minus that, an unfused sum gives 0 where an fma gives 2^-24
    a = F(1.0) + F(2.0 ** -12)
    t = entry((-(1.0 + 2.0 ** -11), 0.0, 0.0), (0.0, 0.0, 1.0), dodx=(float(a), 0.0, 0.0))
    o, _ = ref.jitter(t, float(a), 0.0)
    assert o[0, 0, 0] == F(0.0)


def test_offset_zero_leaves_the_stored_words():
    t = entry((1.0, -0.0, 3.0), (-0.0, 0.0, 1.0), dodx=(np.float32(3e38), 1.0, 1.0), dddx=(7.0, 7.0, 7.0), dddy=(1.0, 2.0, 3.0))
    o, d = ref.jitter(t, 0.0, 0.0)
    assert o.view(np.uint32).tolist() == t[..., 0:3].view(np.uint32).tolist() and d.view(np.uint32).tolist() == t[..., 4:7].view(np.uint32).tolist()
    assert np.signbit(d[0, 0, 0]) and np.signbit(o[0, 0, 1])
    o, d = ref.jitter(t, -0.0, 0.0)   # -0.0 == 0
    assert np.signbit(d[0, 0, 0])
    # ... where any other offset adds: -0.0 + 0 * 7 = +0.0
    _, d = ref.jitter(entry((0, 0, 0), (-0.0, 0.0, 1.0)), 1.0, 0.0)
    assert not np.signbit(d[0, 0, 0])


def test_the_guard_puts_the_stored_ray_back():
    t = entry((1.0, 2.0, 3.0), (1.0, 0.0, 0.0), dodx=(5.0, 0.0, 0.0), dddx=(-1.0, 0.0, 0.0))
    o, d = ref.jitter(t, 1.0, 0.0)
    assert d[0, 0].tolist() == [0.0, 0.0, 0.0] and o[0, 0].tolist() == [6.0, 2.0, 3.0]
    o, d = ref.rays(t, 1.0, 0.0)
    assert d[0, 0].tolist() == [1.0, 0.0, 0.0] and o[0, 0].tolist() == [1.0, 2.0, 3.0]   # origin and direction both
    o, d = ref.rays(t, 0.5, 0.0)
    assert d[0, 0].tolist() == [0.5, 0.0, 0.0] and o[0, 0].tolist() == [3.5, 2.0, 3.0]
    # an overflowing origin is degenerate too
    t = entry((3e38, 0.0, 0.0), (0.0, 0.0, 1.0), dodx=(3e38, 0.0, 0.0))
    o, d = ref.rays(t, 1.0, 0.0)
    assert o[0, 0, 0] == F(3e38)
    assert ref.plain_table(t, 1.0, 0.0).shape == (1, 1, 8)


# ---- raytracer_amd.rays.footprints -----------------------------------------------------------------------------------------------------------------------
OFFSETS = [(0.0, 0.0), (0.5, -0.25), (-1.0, 1.0), (2.0, 0.0), (0.0, -2.0), (1.3, 1.5), (-1.4, -1.4)]   # |o| <= 2


def transform():
    import raytracer_amd as ra
    return ra.transform_from_euler((0.3, 1.0, -2.0), (0.2, -0.4, 0.1))


def test_orthographic_footprints_reproduce_the_builder():
    """the map is exactly linear.  Budget in units of ulp(max |coordinate|): the stored origin carries 1/2 (its own rounding), each derivative 1 (the
    difference of two rounded values), weighted by |sx|, |sy| <= 2; the model's two products and two sums round 1/2 each; the builder's answer 1/2:
    1/2 + 2 + 2 + 2 + 1/2 = 7, held to 8."""
    from raytracer_amd import rays
    w, h, m = 37, 23, transform()
    table = rays.footprints(rays.orthographic, w, h, m, 3.0)
    assert table.shape == (h, w, 32) and table.dtype == np.float32
    ulp = np.spacing(np.abs(table[..., 0:3]).max().astype(np.float32))
    for o in OFFSETS:
        want_o, want_d = rays.orthographic(w, h, m, 3.0, sample_offset=o)
        got_o, got_d = ref.jitter(table, *o)
        assert np.abs(got_o.astype(np.float64) - want_o).max() <= 8 * ulp, o
        assert np.array_equal(got_d, want_d), o   # parallel rays: no direction derivative at all
    assert not table[..., 16:23].any()
    right, up = np.asarray(m, dtype=np.float64).reshape(4, 4)[0, :3], np.asarray(m, dtype=np.float64).reshape(4, 4)[1, :3]
    assert np.allclose(table[..., 24:27], right / np.linalg.norm(right), atol=1e-6) and np.allclose(table[..., 28:31], up / np.linalg.norm(up), atol=1e-6)
    a = rays.footprints(rays.orthographic, w, h, m, 3.0, aperture=0.25, focal_distance=7.0)
    assert (a[..., 3] == F(0.25)).all() and (a[..., 7] == F(7.0)).all() and (table[..., 3] == 0).all() and (table[..., 7] == 1).all()
    with pytest.raises(ValueError):
        rays.footprints(rays.orthographic, w, h, m, 3.0, sample_offset=(0.1, 0.1))
    with pytest.raises(ValueError):
        rays.footprints(rays.hemisphere_probe, np.zeros((1, 3)), np.ones((1, 3)), 4)


def angle(a, b):
    a = a.astype(np.float64) / np.linalg.norm(a.astype(np.float64), axis=-1, keepdims=True)
    b = b.astype(np.float64) / np.linalg.norm(b.astype(np.float64), axis=-1, keepdims=True)
    return np.arctan2(np.linalg.norm(np.cross(a, b), axis=-1), np.einsum("...k,...k->...", a, b))


def neighbour_angle(d, valid=None):
    """the largest angle between the directions of horizontally or vertically neighbouring pixels (both `valid`)"""
    ax, ay = angle(d[:, 1:], d[:, :-1]), angle(d[1:], d[:-1])
    if valid is not None:
        ax, ay = ax[valid[:, 1:] & valid[:, :-1]], ay[valid[1:] & valid[:-1]]
    return max(ax.max(), ay.max())


@pytest.mark.parametrize("projection", ["panorama", "fisheye"])
def test_angular_footprints_are_first_order(projection):
    """The angle between the model's direction at offset o and the builder's stays below (|o| * theta)^2, theta the largest angle between neighbouring
    pixels: a unit direction that turns by at most theta per pixel has a second derivative of at most theta^2 per pixel^2 in every direction, so the
    first-order footprint's remainder is at most |o|^2 theta^2 / 2 -- the bound leaves a factor two, which also covers float32 storage (1e-7) and the
    central difference's third-order term.  The fisheye is smooth only INSIDE its image circle (outside, the builder repeats the axis ray: a jump, not a
    slope), so there the bound is held for the pixels whose samples stay inside at every |o| <= 2 -- at least 2 * sqrt(2) pixels off the circle -- and
    theta is taken among those."""
    from raytracer_amd import rays
    w, h, m = 48, 30, transform()
    if projection == "panorama":
        build, args, valid = rays.panorama, (w, h, m), np.ones((h, w), dtype=bool)
    else:
        build, args = rays.fisheye, (w, h, m, np.radians(170.0))
        x = (2.0 * (np.arange(w) + 0.5) / w - 1.0) * (w / min(w, h))
        y = (2.0 * (np.arange(h) + 0.5) / h - 1.0) * (h / min(w, h))
        r = np.sqrt(x[None, :] ** 2 + y[:, None] ** 2)
        valid = r + 2.0 * np.sqrt(2.0) * (2.0 / min(w, h)) <= 1.0   # a pixel is 2 / shorter wide in these units
        assert valid.sum() > 300
    table = rays.footprints(build, *args)
    theta = neighbour_angle(table[..., 4:7], valid)
    assert 0.01 < theta < 0.3
    worst = 0.0
    for o in OFFSETS[1:]:
        _, want = build(*args, sample_offset=o)
        _, got = ref.jitter(table, *o)
        err = angle(got, want)[valid].max()
        bound = (np.hypot(*o) * theta) ** 2
        print("%s offset %r: angle %.3e, bound %.3e" % (projection, o, err, bound))
        assert err < bound, (o, err, bound)
        worst = max(worst, err / bound)
    assert worst > 1e-3   # (the bound is of the error's order, not vacuous)
    # lens axes: unit length, perpendicular to the stored direction and to each other -- at every pixel, the panorama's poles and the fisheye's outside included
    d, u, v = table[..., 4:7].astype(np.float64), table[..., 24:27].astype(np.float64), table[..., 28:31].astype(np.float64)
    for axis in (u, v):
        assert np.abs(np.linalg.norm(axis, axis=-1) - 1.0).max() < 1e-6
        assert np.abs(np.einsum("...k,...k->...", axis, d)).max() < 1e-6
    assert np.abs(np.einsum("...k,...k->...", u, v)).max() < 1e-6
    # where the ray looks along the transform's forward axis the lens plane is the camera's: (right, up)
    rows = np.asarray(m, dtype=np.float64).reshape(4, 4)
    lu, lv = rays._lens_axes(rows[2:3, :3], rows[0, :3], rows[1, :3])
    assert np.allclose(lu[0], rows[0, :3], atol=1e-12) and np.allclose(lv[0], rows[1, :3], atol=1e-12)
    # and at the poles (d along up) the fallback holds
    lu, lv = rays._lens_axes(np.array([rows[1, :3], -rows[1, :3]]), rows[0, :3], rows[1, :3])
    assert np.allclose(np.linalg.norm(lu, axis=-1), 1.0) and np.allclose(np.einsum("ik,k->i", lu, rows[1, :3]), 0.0, atol=1e-12)
