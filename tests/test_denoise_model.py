"""The a-trous filter's NumPy model (tests/denoise_ref.py, the specification of include/rtgpu.h's rtgpu_filter_atrous) has the properties the
filter is meant to have.  No GPU: the device is held to the model bit for bit in tests/test_gpu_denoise.py."""
import numpy as np

import denoise_ref as ref

F = np.float32


def words(a):
    return np.ascontiguousarray(a).view(np.uint32)


def test_host_constants():
    inv_n, inv_p, inv_c = ref.host_constants(5, 2.0, 0.25, 0.5)
    assert inv_n == F(16.0) and inv_p == F(4.0) and [float(v) for v in inv_c] == [0.25, 1.0, 4.0, 16.0, 64.0]
    assert all(v.dtype == F for v in [inv_n, inv_p] + inv_c)


def test_an_edge_between_two_orientations_stops_the_filter_exactly():
    """two half-planes, normals (1, 0, 0) and (0, 1, 0): |dn|^2 = 2, sigmaNormal = 0.25 -> x = 32 >= 16, the falloff is exactly 0 across the edge; the
    colours are exactly 0 and 1, and within a half-plane sum(w * 1) / sum(w) repeats the same additions above and below the bar"""
    h, w = 40, 48
    left = np.zeros((h, w), dtype=bool)
    left[:, :19] = True
    normal = np.zeros((3, h, w), dtype=F)
    normal[0][left], normal[1][~left] = 1.0, 1.0
    color = np.zeros((h, w, 3), dtype=F)
    color[~left] = 1.0
    depth = np.ones((h, w), dtype=F)
    position = np.zeros((3, h, w), dtype=F)
    out = ref.atrous(color, depth, normal, position, iterations=5, sigma_color=1.0, sigma_normal=0.25, sigma_plane=1.0, demodulate=False)
    assert np.array_equal(words(out), words(color))
    # the control: one orientation, and the edge in the colours bleeds
    normal[:] = 0.0
    normal[0] = 1.0
    bled = ref.atrous(color, depth, normal, position, iterations=5, sigma_color=100.0, sigma_normal=0.25, sigma_plane=1.0, demodulate=False)
    assert not np.array_equal(words(bled), words(color)) and 0.0 < bled[20, 19, 0] < 1.0


def test_invalid_pixels_pass_through_and_touch_nothing():
    f = ref.random_frame(37, 23, seed=5)
    miss = ~np.isfinite(f["depth"])
    assert 20 < miss.sum() < miss.size // 4
    args = dict(iterations=5, sigma_color=4.0, sigma_normal=0.5, sigma_plane=0.2)
    out = ref.atrous(**f, **args)
    assert np.array_equal(words(out[miss]), words(f["color"][miss]))         # (their albedo is 0: d = 1, and colorScale is 1)
    assert not np.array_equal(words(out[~miss]), words(f["color"][~miss]))
    rng = np.random.default_rng(9)
    g = {k: v.copy() for k, v in f.items()}
    g["color"][miss] = rng.random((int(miss.sum()), 3), dtype=F) * F(100.0)
    g["depth"][miss] = np.where(rng.random(int(miss.sum())) < 0.5, np.inf, np.nan).astype(F)
    for name in ("normal", "position", "albedo"):
        g[name][:, miss] = rng.normal(size=(3, int(miss.sum()))).astype(F)
    g["position"][0][miss] = np.nan
    other = ref.atrous(**g, **args)
    assert np.array_equal(words(other[~miss]), words(out[~miss]))
    # (NaN depth is invalid too, and an invalid pixel's colour goes through prepare and finish only)
    d = np.where(g["albedo"] > F(1e-3), g["albedo"], F(1.0)).astype(F)
    expected = np.stack([(g["color"][..., k] / d[k]) * d[k] for k in range(3)], axis=-1)
    assert np.array_equal(words(other[miss]), words(expected[miss]))


def test_one_level_reduces_white_noise_as_the_b3_kernel_does():
    """constant guides, sigmas so large that every falloff is 1 to within rounding: one level is the separable B3 blur {1/16, 1/4, 3/8, 1/4, 1/16}, whose
    output variance on white noise is (sum h^2)^2 = 0.2734375^2 = 0.0748 of the input's.  +-15 %: the interior holds 3600 output samples, correlated over
    the kernel's footprint (some 3600 / 13 independent ones: 1 / sum of the squared autocorrelation), so one standard deviation of the variance estimate
    is about sqrt(2 * 13 / 3600) = 8.5 %; this seed gives 0.0766, +2.4 %."""
    h = w = 64
    rng = np.random.default_rng(1234)
    color = np.repeat(rng.normal(size=(h, w, 1)).astype(F), 3, axis=2)
    normal = np.zeros((3, h, w), dtype=F)
    normal[2] = 1.0
    out = ref.atrous(color, np.ones((h, w), dtype=F), normal, np.zeros((3, h, w), dtype=F), iterations=1, sigma_color=1e6, sigma_normal=1e6, sigma_plane=1e6,
                     demodulate=False)
    inner = (slice(2, h - 2), slice(2, w - 2))
    ratio = float(out[inner][..., 0].astype(np.float64).var() / color[inner][..., 0].astype(np.float64).var())
    expected = (0.375 ** 2 + 2 * 0.25 ** 2 + 2 * 0.0625 ** 2) ** 2
    print("variance ratio %.5f, the B3 kernel's %.5f" % (ratio, expected))
    assert abs(expected - 0.0748) < 1e-4 and abs(ratio / expected - 1.0) < 0.15


def test_demodulation_keeps_texture_detail():
    """a checkerboard albedo under constant irradiance: demodulated, the filter sees a constant image and returns the input to within rounding;
    not demodulated, the colour term is all that keeps the squares apart and a wide colour sigma blurs them"""
    h, w = 24, 24
    ys, xs = np.mgrid[0:h, 0:w]
    albedo = np.repeat((np.where((xs // 4 + ys // 4) % 2 == 0, 0.8, 0.2).astype(F))[None], 3, axis=0)
    color = np.moveaxis(albedo * F(1.5), 0, -1).copy()
    normal = np.zeros((3, h, w), dtype=F)
    normal[2] = 1.0
    args = dict(depth=np.ones((h, w), dtype=F), normal=normal, position=np.zeros((3, h, w), dtype=F), iterations=3, sigma_color=50.0)
    kept = ref.atrous(color, albedo=albedo, demodulate=True, **args)
    assert np.abs(kept - color).max() < 1e-6
    blurred = ref.atrous(color, albedo=None, demodulate=False, **args)
    assert np.abs(blurred - color).max() > 0.1
