"""The last step of every frame on the DEVICE -- k_postprocess, k_blur_lines, k_postprocess_bloom (csrc/rt_post.inl) and postProcessPixel with its
helpers (csrc/rt_device_core.h) -- held to the reference's own vectors at float level and to the oracle on crafted frames.

  * vectors: rtgpu_kat_postprocess over postprocess_kat.bin and postprocess_edges_kat.bin, rtgpu_kat_blur over bloom_kat.bin and bloom_edges_kat.bin
    (written by the reference's code, oracle/ref_harness/kat_gen.cpp).  Against the oracle every 8-bit word and every float before quantisation is
    identical under all four tone mappers; against the reference the terms of tests/test_oracle_kat.py hold (Clamped / Reinhard exact; the two operators
    behind the vendor-specific _mm_rcp_ps seed within one LSB on at most 0.5 % of the channels).  The blur: every lattice float and the checksum.
  * crafted frames through rtgpu_postprocess_from: zeros, denormals, huge values, infinities, NaN and negative channels at the first pixel, the last
    pixel and a row end, all tone mappers, dithering up to a strength that overflows the conversion to integer; with bloom, fireflies and a single
    +inf / NaN pixel at the smallest frame the blur admits and at a tall one.  The 8-bit frame is the oracle's.
  * the sizes bloom refuses, and the statuses of the two hooks.

Floats compare bit for bit where the expected one is not NaN and as "both NaN" where it is (x86 and the GPU produce different NaN patterns)."""
import ctypes as C

import numpy as np
import pytest

import kat_io
import oracle_lib

pytestmark = pytest.mark.gpu

INVALID_ARGUMENT, UNSUPPORTED = -1, -6
SENTINEL = 0xDEADBEEF


@pytest.fixture(scope="module")
def ctx(built):
    import raytracer_amd as ra
    lib = ra.rtgpu_lib()
    c = C.c_void_p()
    assert lib.rtgpu_create(0, C.byref(c)) == 0, lib.rtgpu_last_error()
    yield lib, c
    lib.rtgpu_destroy(c)


def ptr(a):
    return a.ctypes.data_as(C.c_void_p)


def make_params(tonemapper, dithering=0.0, seed=0, bloom=0.0, exposure=0.0, contrast=0.8, saturation=0.98, num_passes=1):
    import raytracer_amd as ra
    p = ra.RtPostprocessParams()
    for k in range(4):
        p.colorFilter[k] = (1.0, 0.9, 1.1, 1.0)[k]
    p.exposure, p.contrast, p.saturation, p.ditheringStrength, p.bloomFactor = exposure, contrast, saturation, dithering, bloom
    p.tonemapper, p.numPasses, p.ditherSeed = tonemapper, num_passes, seed
    return p


# ---- vectors --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", kat_io.POSTPROCESS_FILES)
def test_device_postprocess_matches_oracle_and_reference_vectors(ctx, name):
    lib, c = ctx
    recs = kat_io.load_postprocess(name)
    params, rgb = kat_io.postprocess_arrays(recs)
    n = len(recs)
    bgr, tone = np.full(n, SENTINEL, dtype=np.uint32), np.full((n, 3), -7.0, dtype=np.float32)
    assert lib.rtgpu_kat_postprocess(c, params, ptr(rgb), n, ptr(bgr), ptr(tone)) == 0, lib.rtgpu_last_error()
    # the oracle: identical, all four operators, no allowance
    obgr, otone = np.zeros(n, dtype=np.uint32), np.zeros((n, 3), dtype=np.float32)
    oracle_lib.lib().rto_postprocess_records(params, ptr(rgb), C.c_uint32(n), ptr(obgr), ptr(otone))
    bad = kat_io.bit_mismatch(otone, tone)
    print("%s: vs oracle %d floats, %d words differ" % (name, int(bad.sum()), int((bgr != obgr).sum())))
    assert not bad.any(), "%d floats differ from the oracle's, first record %d" % (int(bad.sum()), int(np.nonzero(bad.any(axis=1))[0][0]))
    assert np.array_equal(bgr, obgr), "record %d" % int(np.nonzero(bgr != obgr)[0][0])
    # the reference: the terms of test_oracle_kat.py::test_postprocess_matches_reference
    tonemapper = np.array([p.tonemapper for p in params])
    exact = tonemapper <= 1
    bad = kat_io.bit_mismatch(recs["toneMapped"], tone)
    assert not bad[exact].any(), "%d floats of the exact operators differ from the reference's" % int(bad[exact].sum())
    assert np.array_equal(bgr[exact], recs["bgr"][exact])
    d = np.stack([np.abs(((bgr[~exact] >> s) & 255).astype(np.int64) - ((recs["bgr"][~exact] >> s) & 255).astype(np.int64)) for s in (0, 8, 16)], axis=1)
    print("%s: vs reference, approximate operators: %d of %d channels off by one, largest difference %d" % (name, int((d == 1).sum()), d.size, int(d.max())))
    assert d.max() <= 1
    assert d.sum() <= 0.005 * d.size, (int(d.sum()), d.size)
    assert np.array_equal(np.isnan(tone), np.isnan(recs["toneMapped"]))
    # outToneMapped is optional and changes nothing
    again = np.full(n, SENTINEL, dtype=np.uint32)
    assert lib.rtgpu_kat_postprocess(c, params, ptr(rgb), n, ptr(again), None) == 0
    assert np.array_equal(again, bgr)


@pytest.mark.parametrize("name", kat_io.BLOOM_FILES)
def test_device_blur_matches_reference_vectors(ctx, name):
    lib, c = ctx
    cases = kat_io.load_bloom(name)
    assert len(cases) == (8 if "edges" in name else 3)
    for case in cases:
        img, sigma = case["image"].copy(), case["sigma0"]
        for number, level in enumerate(case["levels"]):
            assert lib.rtgpu_kat_blur(c, ptr(img), case["w"], case["h"], sigma) == 0, lib.rtgpu_last_error()
            sigma = float(np.float32(sigma) * np.float32(2.5))
            kat_io.check_blur_level(img, level, case["step"], "%s %dx%d edit %d level %d" % (name, case["w"], case["h"], case["edit"], number))


# ---- crafted frames -------------------------------------------------------------------------------------------------------------------------
def crafted_frame(w, h, special, seed):
    """ordinary values in [0, 2) with a few bright ones; `special` at the first pixel (all channels), at the last pixel (one channel) and at the end of
    the middle row (the two other channels)"""
    rng = np.random.RandomState(seed)
    img = (rng.random_sample((h, w, 3)) * 2.0).astype(np.float32)
    img[rng.random_sample((h, w)) < 0.02] *= np.float32(300.0)
    k = seed % 3
    img[0, 0, :] = special
    img[h - 1, w - 1, k] = special
    img[h // 2, w - 1, (k + 1) % 3] = special
    img[h // 2, w - 1, (k + 2) % 3] = special
    return img


def device_frame(lib, c, img, p):
    h, w = img.shape[:2]
    out = np.full((h, w), SENTINEL, dtype=np.uint32)
    assert lib.rtgpu_postprocess_from(c, C.byref(p), ptr(img), ptr(out)) == 0, lib.rtgpu_last_error()
    return out


def oracle_frame(img, p):
    h, w = img.shape[:2]
    out = np.zeros((h, w), dtype=np.uint32)
    if p.bloomFactor > 0.0:
        assert oracle_lib.lib().rto_postprocess_bloom(ptr(img), C.c_uint32(w), C.c_uint32(h), C.byref(p), ptr(out)) == 0
    else:
        oracle_lib.lib().rto_postprocess(ptr(img), C.c_uint32(w), C.c_uint32(h), C.byref(p), ptr(out))
    return out


@pytest.mark.parametrize("size", [(1, 1), (67, 41)])
def test_crafted_frames_match_the_oracle(ctx, size):
    """every special value x all four operators x dither seeds {0, 17, 0xFFFFFFFF} x strengths {0, 0.005, 1e10}; at 1e10 the dithered channel times
    255 leaves the int32 range, where _mm_cvttps_epi32 gives INT_MIN (black) and a saturating conversion would give white"""
    lib, c = ctx
    w, h = size
    assert lib.rtgpu_resize(c, w, h) == 0, lib.rtgpu_last_error()
    for s, special in enumerate(kat_io.POST_SPECIALS):
        img = crafted_frame(w, h, special, 100 + s)
        for tonemapper in range(4):
            for seed in (0, 17, 0xFFFFFFFF):
                for strength in (0.0, 0.005, 1e10):
                    p = make_params(tonemapper, dithering=strength, seed=seed, num_passes=1 + s % 2)
                    got, want = device_frame(lib, c, img, p), oracle_frame(img, p)
                    assert np.array_equal(got, want), "special %r operator %d seed %d strength %g: %d pixels differ, first %s: device %08x oracle %08x" % (
                        float(special), tonemapper, seed, strength, int((got != want).sum()), np.argwhere(got != want)[0],
                        int(got[tuple(np.argwhere(got != want)[0])]), int(want[tuple(np.argwhere(got != want)[0])]))


def test_overflowing_conversion_is_black_like_the_reference(ctx):
    """_mm_cvttps_epi32 gives INT_MIN for NaN and for anything outside [-2^31, 2^31); the clamp to [0, 255] then makes it 0.  One pixel, no dithering
    noise of either sign can bring 1e10 * noise back into range except |noise| < 8.4e-4: the channels come out 0 or, in range and positive, 255."""
    lib, c = ctx
    assert lib.rtgpu_resize(c, 4, 2) == 0
    img = np.full((2, 4, 3), 0.5, dtype=np.float32)
    p = make_params(0, dithering=1e10, seed=3)
    got = device_frame(lib, c, img, p)
    assert np.array_equal(got, oracle_frame(img, p))
    channels = np.stack([(got >> s) & 255 for s in (16, 8, 0)], axis=-1)
    assert np.isin(channels, (0, 255)).all()
    assert (channels == 0).sum() >= 20      # positive and negative overflow alike: black (24 channels, |noise| < 8.4e-4 has probability < 1e-3)


@pytest.mark.parametrize("size", [(196, 196), (200, 452)])
def test_crafted_frames_with_bloom_match_the_oracle(ctx, size):
    """the smallest frame bloom admits and a tall one; fireflies; one +inf pixel; one NaN pixel.  inf - inf in a box blur's running sum poisons the
    rest of the pixel's line, the vertical pass every column it reached, the next level whatever those touch: the poisoned area must be the oracle's, in the frame and after the first level alone"""
    lib, c = ctx
    w, h = size
    assert lib.rtgpu_resize(c, w, h) == 0, lib.rtgpu_last_error()
    clean = kat_io.bloom_input(w * h * 3).reshape(h, w, 3).copy()     # 1 / 64 of the floats are fireflies of up to 400
    frames = {"finite": clean}
    for label, bits in (("inf", 0x7F800000), ("nan", 0x7FC00000)):
        img = clean.copy()
        img[h // 3, w // 2, 1] = np.array([bits], dtype=np.uint32).view(np.float32)[0]
        frames[label] = img
    for bloom, tonemapper in ((0.35, 3), (1.0, 2)):
        p = make_params(tonemapper, dithering=0.005, seed=17, bloom=bloom)
        results = {}
        for label, img in frames.items():
            got, want = device_frame(lib, c, img, p), oracle_frame(img, p)
            assert np.array_equal(got, want), "%s bloom %g: %d pixels differ" % (label, bloom, int((got != want).sum()))
            results[label] = (got, want)
        plain = device_frame(lib, c, clean, make_params(tonemapper, dithering=0.005, seed=17, bloom=0.0))
        assert np.count_nonzero(plain != results["finite"][0]) > 0.5 * w * h     # the blur reaches the picture
        for label in ("inf", "nan"):
            poisoned = results[label][0] != results["finite"][0]
            expected = results[label][1] != results["finite"][1]
            assert np.array_equal(poisoned, expected)
            print("%dx%d bloom %g %s: %d of %d pixels poisoned (oracle %d)" % (w, h, bloom, label, int(poisoned.sum()), w * h, int(expected.sum())))
            assert poisoned.any()
            assert poisoned[h // 3, w // 2]
            assert not poisoned.all() or expected.all()
    # five levels of up to 195 pixels spread one pixel over the whole frame; after the first level (sigma 2) the area is a band of rows and columns,
    # and it must be the oracle's word for word
    for label in ("inf", "nan"):
        got, want = frames[label].copy(), frames[label].copy()
        assert lib.rtgpu_kat_blur(c, ptr(got), w, h, 2.0) == 0, lib.rtgpu_last_error()
        assert oracle_lib.lib().rto_gaussian_blur(ptr(want), C.c_uint32(w), C.c_uint32(h), C.c_float(2.0), C.c_uint32(8)) == 0
        assert np.array_equal(np.isnan(got), np.isnan(want)) and not kat_io.bit_mismatch(want, got).any()
        assert 0 < np.isnan(got).sum() < got.size // 3 and not np.isnan(got[..., 0]).any() and not np.isnan(got[..., 2]).any(), label


# ---- refusals -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", [(195, 196), (196, 195), (198, 196), (4100, 196)])
def test_sizes_bloom_refuses(ctx, size):
    lib, c = ctx
    w, h = size
    assert lib.rtgpu_resize(c, w, h) == 0, lib.rtgpu_last_error()
    img = np.full((h, w, 3), 0.25, dtype=np.float32)
    out = np.full((h, w), SENTINEL, dtype=np.uint32)
    p = make_params(3, bloom=0.35)
    assert lib.rtgpu_postprocess_from(c, C.byref(p), ptr(img), ptr(out)) == UNSUPPORTED
    assert b"bloom" in lib.rtgpu_last_error()
    assert (out == SENTINEL).all()
    p.bloomFactor = 0.0
    assert lib.rtgpu_postprocess_from(c, C.byref(p), ptr(img), ptr(out)) == 0, lib.rtgpu_last_error()
    assert np.array_equal(out, oracle_frame(img, p)) and (out != SENTINEL).all()


def test_hook_statuses(ctx):
    lib, c = ctx
    rgb, bgr, tone = np.full((4, 3), 0.5, dtype=np.float32), np.full(4, SENTINEL, dtype=np.uint32), np.full((4, 3), -7.0, dtype=np.float32)
    import raytracer_amd as ra
    params = (ra.RtPostprocessParams * 4)(*[make_params(t) for t in range(4)])
    assert lib.rtgpu_kat_postprocess(c, None, ptr(rgb), 4, ptr(bgr), ptr(tone)) == INVALID_ARGUMENT
    assert lib.rtgpu_kat_postprocess(c, params, None, 4, ptr(bgr), ptr(tone)) == INVALID_ARGUMENT
    assert lib.rtgpu_kat_postprocess(c, params, ptr(rgb), 4, None, ptr(tone)) == INVALID_ARGUMENT
    assert lib.rtgpu_kat_postprocess(c, None, None, 0, None, None) == 0          # nothing to do
    params[2].tonemapper = 4
    assert lib.rtgpu_kat_postprocess(c, params, ptr(rgb), 4, ptr(bgr), ptr(tone)) == INVALID_ARGUMENT and b"tonemapper" in lib.rtgpu_last_error()
    params[2].tonemapper = 2
    params[3].numPasses = 0
    assert lib.rtgpu_kat_postprocess(c, params, ptr(rgb), 4, ptr(bgr), ptr(tone)) == INVALID_ARGUMENT and b"numPasses" in lib.rtgpu_last_error()
    assert (bgr == SENTINEL).all() and (tone == -7.0).all()                      # a refused call writes nothing
    params[3].numPasses = 1
    assert lib.rtgpu_kat_postprocess(c, params, ptr(rgb), 4, ptr(bgr), ptr(tone)) == 0 and (bgr != SENTINEL).all()

    assert lib.rtgpu_kat_blur(c, None, 8, 8, 1.3) == INVALID_ARGUMENT
    for w, h, sigma, status in ((6, 8, 1.3, UNSUPPORTED),        # width not a multiple of 4
                                (8, 7, 1.3, UNSUPPORTED),        # 7 = 2 * wu + 1 at sigma 1.3 (wu = 3): not larger than the window
                                (4, 8, 1.3, UNSUPPORTED),
                                (4100, 8, 1.3, UNSUPPORTED), (8, 4097, 1.3, UNSUPPORTED),
                                (64, 48, 31.25, UNSUPPORTED),    # the frame's fourth level: wu = 39, 79 pixels
                                (0, 8, 1.3, INVALID_ARGUMENT), (8, 8, 0.0, INVALID_ARGUMENT), (8, 8, float("nan"), INVALID_ARGUMENT)):
        img = kat_io.bloom_input(max(w, 1) * max(h, 1) * 3)
        before = img.copy()
        assert lib.rtgpu_kat_blur(c, ptr(img), w, h, sigma) == status, (w, h, sigma)
        assert np.array_equal(img, before), (w, h, sigma)
    img = kat_io.bloom_input(8 * 8 * 3)
    before = img.copy()
    assert lib.rtgpu_kat_blur(c, ptr(img), 8, 8, 1.3) == 0 and not np.array_equal(img, before)
