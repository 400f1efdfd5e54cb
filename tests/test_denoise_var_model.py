"""The variance-guided filter's NumPy model (tests/denoise_var_ref.py, the specification of include/rtgpu.h's rtgpu_filter_atrous_var) has the properties
the filter is meant to have.  They are exact properties of the model: no tolerances.  No GPU: the device is held to the model bit for bit in
tests/test_gpu_denoise_var.py."""
import numpy as np

import denoise_var_ref as ref

F = np.float32


def words(a):
    return np.ascontiguousarray(a).view(np.uint32)


def flat(h, w):
    """one flat, all-valid geometry: a single normal, positions on its plane"""
    normal = np.zeros((3, h, w), dtype=F)
    normal[2] = 1.0
    ys, xs = np.mgrid[0:h, 0:w]
    position = np.stack([xs * F(0.01), ys * F(0.01), np.zeros((h, w))]).astype(F)
    return dict(depth=np.ones((h, w), dtype=F), normal=normal, position=position)


def two_colours(h, w, edge):
    color = np.zeros((h, w, 3), dtype=F)
    color[:, edge:] = 1.0
    return color


def test_host_constants():
    inv_n, inv_p, sl2 = ref.host_constants(4.0, 0.25, 0.5)
    assert inv_n == F(16.0) and inv_p == F(4.0) and sl2 == F(16.0) and all(v.dtype == F for v in (inv_n, inv_p, sl2))
    assert ref.lum([F(1.0), F(1.0), F(1.0)]) == F(1.0) and ref.lum([F(4.0), F(0.0), F(0.0)]) == F(1.0) and ref.lum([F(0.0), F(2.0), F(0.0)]) == F(1.0)


def test_zero_variance_keeps_an_edge_in_the_colours_exactly():
    """colours 0 and 1 on one flat geometry, color_half = color / 2: v = 0 everywhere, denom = varianceFloor = 1e-10, a tap across the edge has
    xc = 1 / 1e-10 >= 16 and weight exactly 0, and a tap on the same side has x = 0: sum(w * 1) / sum(w) repeats the same additions above and below the bar"""
    h, w, edge = 40, 48, 19
    color = two_colours(h, w, edge)
    out, v = ref.atrous_var(color, color * F(0.5), iterations=5, demodulate=False, **flat(h, w))
    assert np.array_equal(words(out), words(color))
    assert not v.any()


def test_a_large_variance_and_nothing_else_opens_that_edge():
    """the same frame with color_half = (color + 1) / 2: b = color + 1, e = -1, v = 1 everywhere, denom = 16 + 1e-10, a tap across the edge has xc = 1 / 16"""
    h, w, edge = 40, 48, 19
    color = two_colours(h, w, edge)
    half = ((color + F(1.0)) * F(0.5)).astype(F)
    one, v1 = ref.atrous_var(color, half, iterations=1, demodulate=False, **flat(h, w))
    assert ((one[:, edge - 1] > 0.0) & (one[:, edge - 1] < 1.0)).all() and ((one[:, edge] > 0.0) & (one[:, edge] < 1.0)).all()
    assert (v1 < 1.0).all() and (v1 > 0.0).all()
    out, _ = ref.atrous_var(color, half, iterations=5, demodulate=False, **flat(h, w))
    assert ((out[:, edge - 1] > 0.0) & (out[:, edge - 1] < 1.0)).all() and ((out[:, edge] > 0.0) & (out[:, edge] < 1.0)).all()


def test_invalid_pixels_keep_colour_and_variance_and_touch_nothing():
    f = ref.random_frame_var(37, 23, seed=5)
    miss = ~np.isfinite(f["depth"])
    assert 20 < miss.sum() < miss.size // 4
    args = dict(iterations=5, sigma_lum=4.0, sigma_normal=0.5, sigma_plane=0.2)
    out, v = ref.atrous_var(**f, **args)
    assert np.array_equal(words(out[miss]), words(f["color"][miss]))         # (their albedo is 0: d = 1, and colorScale is 1)
    assert np.array_equal(words(v[miss]), words(np.zeros(int(miss.sum()), dtype=F)))
    assert not np.array_equal(words(out[~miss]), words(f["color"][~miss])) and v[~miss].any()
    # whatever an invalid pixel holds, the valid ones come out the same: it is in nobody's window and nobody's taps
    rng = np.random.default_rng(9)
    g = {k: a.copy() for k, a in f.items()}
    g["color"][miss] = rng.random((int(miss.sum()), 3), dtype=F) * F(100.0)
    g["color_half"][miss] = rng.random((int(miss.sum()), 3), dtype=F) * F(100.0)
    g["color_half"][..., 1][miss] = np.nan
    for name in ("normal", "position"):
        g[name][:, miss] = rng.normal(size=(3, int(miss.sum()))).astype(F)
    other, ov = ref.atrous_var(**g, **args)
    assert np.array_equal(words(other[~miss]), words(out[~miss])) and np.array_equal(words(ov), words(v))
    assert np.array_equal(words(other[miss]), words(g["color"][miss]))


def test_the_variance_of_a_flat_frame_shrinks_as_the_sum_of_squared_weights():
    """uniform colour, uniform variance, flat geometry: every tap has x = 0 and w = h_i * h_j, so one level leaves sum(w^2 * v) / (sum w)^2 -- the
    same additions in the same order, hence the same bits -- at every pixel whose 25 taps are inside the frame, and that is below v"""
    h, w = 16, 20
    color = np.full((h, w, 3), 0.75, dtype=F)
    half = np.full((h, w, 3), 0.5, dtype=F)   # b = 1, e = -0.25, v = 0.0625
    out, v = ref.atrous_var(color, half, iterations=1, demodulate=False, **flat(h, w))
    v0 = F(0.0625)
    vacc, wsum = F(0.0), F(0.0)
    for j in range(-2, 3):
        for i in range(-2, 3):
            wt = (ref.H_WEIGHTS[abs(i)] * ref.H_WEIGHTS[abs(j)]) * F(1.0)
            vacc = vacc + (wt * wt) * v0
            wsum = wsum + wt
    expected = vacc / (wsum * wsum)
    inner = v[2:h - 2, 2:w - 2]
    assert expected.dtype == F and np.array_equal(words(inner), words(np.full(inner.shape, expected, dtype=F)))
    assert (inner < v0).all() and abs(float(expected) / float(v0) - 0.2734375 ** 2) < 1e-6
    assert np.array_equal(words(out), words(color))
    assert (v < v0).all()   # (at the border fewer taps: less averaging, still some)


def test_a_nan_in_the_half_buffer_leaves_every_other_pixel_finite():
    """v is NaN at that pixel, so g, denom and every weight of its neighbours' are NaN -> 0 through fmax: they keep their colour; a pixel further away
    takes the pixel's (finite) colour as a tap like any other.  The variance is another matter: (w * w) * NaN is NaN whatever w, by the definition's
    operations, and spreads over the taps' reach."""
    f = ref.random_frame_var(37, 23, seed=6, invalid=0.0)
    f["color_half"][11, 17, 1] = np.nan
    out, v = ref.atrous_var(iterations=5, **f)
    assert np.isfinite(out).all()
    clean = dict(f, color_half=np.nan_to_num(f["color_half"], nan=1.0))
    assert not np.array_equal(words(out), words(ref.atrous_var(iterations=5, **clean)[0]))
    assert np.isnan(v[11, 17]) and np.isfinite(v).any()


def test_demodulation_commutes_with_a_power_of_two_albedo():
    """albedo in {1/4, 1/2, 1, 2}: multiplying by it and dividing it out again are exact, so the filter with RT_DENOISE_DEMODULATE over colour * albedo is
    albedo * (the filter over the colour), and the variance is the same"""
    f = ref.random_frame_var(37, 23, seed=7)
    rng = np.random.default_rng(8)
    albedo = np.float32(2.0) ** rng.integers(-2, 2, size=f["albedo"].shape).astype(F)
    lit = {k: (f[k] * np.moveaxis(albedo, 0, -1)).astype(F) for k in ("color", "color_half")}
    args = dict(depth=f["depth"], normal=f["normal"], position=f["position"], iterations=3, color_scale=0.25)
    plain, pv = ref.atrous_var(f["color"], f["color_half"], demodulate=False, **args)
    got, gv = ref.atrous_var(lit["color"], lit["color_half"], albedo=albedo, demodulate=True, **args)
    assert np.array_equal(words(got), words(plain * np.moveaxis(albedo, 0, -1))) and np.array_equal(words(gv), words(pv))
    assert not np.array_equal(words(plain), words(f["color"] * F(0.25)))
