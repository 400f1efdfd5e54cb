"""tests/temporal_ref.py, the NumPy float32 model of temporal accumulation (include/rtgpu.h: rtgpu_temporal_accumulate), held to the properties the operation is
meant to have.  No GPU: the device is held to the model bit for bit in tests/test_gpu_temporal.py."""
import numpy as np
import pytest

import temporal_ref as ref
from denoise_var_ref import lum

F = np.float32
EPS = float(np.finfo(np.float32).eps)
W, H = 16, 8   # powers of two: the affine matrix of an unmoved camera sends pixel x to fx = x exactly


def flat(w=W, h=H, seed=0, shift=(0.0, 0.0)):
    """a plane facing the camera, seen alike by both frames: (guides, the prevWorldToScreen that shifts by `shift` pixels); colours are the caller's"""
    ys, xs = np.mgrid[0:h, 0:w]
    guides = dict(depth=np.full((h, w), 2.0, dtype=F), normal=np.stack([np.zeros((h, w)), np.zeros((h, w)), np.ones((h, w))]).astype(F),
                  position=np.stack([xs, ys, np.full((h, w), 2.0)]).astype(F), object_id=np.ones((h, w), dtype=np.uint32))
    return guides, ref.affine_world_to_screen(w, h, shift)


def copy(guides):
    return {k: v.copy() for k, v in guides.items()}


def frames(count, w=W, h=H, seed=1, sigma=0.5, mean=2.0):
    """independent Gaussian frames around a constant: per frame the full estimate a and the half-sample sum (b / 2), whose error a - b is independent of a's"""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(count):
        a = (mean + rng.normal(scale=sigma, size=(h, w, 3))).astype(F)
        b = (a + rng.normal(scale=sigma, size=(h, w, 3))).astype(F)
        out.append((a, (b * F(0.5)).astype(F)))
    return out


def run(sequence, guides, matrix, **params):
    """the frames accumulated one after the other over the same guides; yields (history, motion, taken, reason) per frame"""
    history = None
    for color, half in sequence:
        history, motion, taken, reason = ref.accumulate(color, half, albedo=None, demodulate=False, history=history, prev_world_to_screen=matrix, **guides, **params)
        yield history, motion, taken, reason


# ---- 1. an unmoved camera: the running mean -------------------------------------------------------------------------------------------------------
def test_an_unmoved_camera_accumulates_the_running_mean():
    guides, matrix = flat()
    sequence = frames(12)
    max_history = 8.0
    total = np.zeros((H, W, 3), dtype=np.float64)
    biggest = max(float(np.abs(a).max()) for a, _ in sequence)
    for i, (history, motion, taken, reason) in enumerate(run(sequence, guides, matrix, alpha_min=1e-6, max_history=max_history)):
        # the length runs 1, 2, 3, ... up to maxHistory, exactly: fx = x, so the tap at the pixel itself has weight 1 and the others 0
        assert np.array_equal(history["length"], np.full((H, W), min(i + 1.0, max_history), dtype=F)), i
        assert not motion.any()
        if i == 0:
            assert (reason == ref.START_NO_HISTORY).all()
        else:
            assert (reason == ref.BLENDED).all() and (taken[:-1, :-1] == 4).all()
        if i < max_history:
            # a blend is a division, a subtraction, a multiplication and an addition: four roundings of at most eps / 2 of values no larger than the largest
            # input, and the error it inherits is scaled by 1 - alpha <= 1; so after i blends at most 2 * i * eps * max|a|, and twice that for slack
            total += sequence[i][0].astype(np.float64)
            assert np.abs(history["a"] - total / (i + 1)).max() <= 4.0 * max(i, 1) * EPS * biggest, i
    # at the cap the history is an exponential average: the last frame weighs 1 / maxHistory


def test_alpha_min_one_returns_the_current_frame():
    guides, matrix = flat()
    sequence = frames(3)
    for i, (history, _, _, reason) in enumerate(run(sequence, guides, matrix, alpha_min=1.0)):
        a, half = sequence[i]
        # h + 1 * (c - h): two roundings, each at most eps / 2 of a value no larger than |c| + |h|
        bound = 2.0 * EPS * float(np.abs(a).max() + np.abs(sequence[max(i - 1, 0)][0]).max())
        assert np.abs(history["a"] - a).max() <= bound and np.abs(history["b"] - half * F(2.0)).max() <= 2.0 * bound
        assert np.array_equal(history["length"], np.full((H, W), min(i + 1.0, 64.0), dtype=F))


def test_demodulation_divides_once_and_history_space_stays_divided():
    guides, matrix = flat()
    rng = np.random.default_rng(5)
    albedo = (rng.random((3, H, W)) * 0.9 + 0.05).astype(F)
    albedo[0, 2, 3] = F(5e-4)   # below 1e-3: d = 1
    (a, half), = frames(1)
    first, _, _, _ = ref.accumulate(a, half, albedo=albedo, demodulate=True, color_scale=0.5, **guides)
    d = np.moveaxis(np.where(albedo > F(1e-3), albedo, F(1.0)), 0, -1)
    assert np.array_equal(first["a"], (a * F(0.5)) / d) and np.array_equal(first["b"], (half * (F(2.0) * F(0.5))) / d)
    assert np.array_equal(ref.remodulate(first["a"], albedo), first["a"] * d)
    second, _, _, _ = ref.accumulate(a, half, albedo=albedo, demodulate=True, color_scale=0.5, history=first, prev_world_to_screen=matrix, **guides)
    assert np.abs(second["a"] - first["a"]).max() <= 4 * EPS * float(np.abs(first["a"]).max())   # the same frame again: the mean stays


# ---- 2. starts --------------------------------------------------------------------------------------------------------------------------------------
def spoil(what):
    cur, matrix = flat()
    prev = copy(cur)
    y, x = 3, 5
    if what == "object id":
        cur["object_id"][y, x] = 2
    elif what == "normal":
        cur["normal"][:, y, x] = (1.0, 0.0, 0.0)
    elif what == "plane":
        cur["position"][2, y, x] += F(1.0)
    elif what == "behind":
        cur["position"][2, y, x] = F(-1.0)
    elif what == "outside":
        cur["position"][0, y, x] = F(100.0)
    elif what == "not a number":
        cur["position"][1, y, x] = np.nan
    elif what == "invalid":
        cur["depth"][y, x] = np.inf
    return cur, prev, matrix, (y, x)


@pytest.mark.parametrize("what, reason", [("object id", ref.START_NO_TAP), ("normal", ref.START_NO_TAP), ("plane", ref.START_NO_TAP), ("behind", ref.START_OFF_SCREEN),
                                          ("outside", ref.START_OFF_SCREEN), ("not a number", ref.START_OFF_SCREEN), ("invalid", ref.START_INVALID)])
def test_each_failed_test_starts_the_pixel(what, reason):
    cur, prev, matrix, at = spoil(what)
    (a0, h0), (a1, h1) = frames(2)
    first, _, _, _ = ref.accumulate(a0, h0, demodulate=False, **prev)
    second, motion, taken, why = ref.accumulate(a1, h1, demodulate=False, history=first, prev_world_to_screen=matrix, **cur)
    assert why[at] == reason and taken[at] == 0 and second["length"][at] == 1.0 and not motion[:, at[0], at[1]].any()
    assert np.array_equal(second["a"][at], a1[at]) and np.array_equal(second["b"][at], h1[at] * F(2.0))
    others = np.ones((H, W), dtype=bool)
    others[at] = False
    assert (why[others] == ref.BLENDED).all() and (second["length"][others] == 2.0).all()
    assert np.isfinite(second["a"]).all()


def test_without_both_id_planes_the_object_test_is_skipped():
    cur, prev, matrix, at = spoil("object id")
    (a0, h0), (a1, h1) = frames(2)
    del cur["object_id"], prev["object_id"]
    first, _, _, _ = ref.accumulate(a0, h0, demodulate=False, **prev)
    second, _, _, why = ref.accumulate(a1, h1, demodulate=False, history=first, prev_world_to_screen=matrix, **cur)
    assert (why == ref.BLENDED).all() and first["object_id"] is None


def test_one_bad_tap_of_four_renormalises_the_other_three():
    cur, matrix = flat(shift=(0.5, 0.5))   # every tap weighs a quarter
    prev = copy(cur)
    y, x = 3, 5
    prev["depth"][y + 1, x + 1] = np.inf
    (a0, h0), (a1, h1) = frames(2)
    first, _, _, _ = ref.accumulate(a0, h0, demodulate=False, **prev)
    first["length"][y, x + 1] = F(4.0)
    second, motion, taken, why = ref.accumulate(a1, h1, demodulate=False, history=first, prev_world_to_screen=matrix, alpha_min=1e-6, **cur)
    assert taken[y, x] == 3 and why[y, x] == ref.BLENDED and (taken[:-1, :-1] >= 3).all() and taken[0, 0] == 4
    assert np.allclose(motion[:, y, x], (0.5, 0.5), atol=1e-5)
    three = (first["a"][y, x].astype(np.float64) + first["a"][y, x + 1] + first["a"][y + 1, x]) / 3.0
    n = (1.0 + 4.0 + 1.0) / 3.0 + 1.0
    assert abs(float(second["length"][y, x]) - n) <= 4 * EPS * n
    assert np.abs(second["a"][y, x] - (three + (a1[y, x] - three) / n)).max() <= 16 * EPS * float(np.abs(a0).max() + np.abs(a1).max())


# ---- 3. the convention: the library's own camera -----------------------------------------------------------------------------------------------------
def unproject(camera, w, h, sample_offset, distance):
    """the points at `distance` along the camera's axis that the primary rays of the pixel grid go through: Camera::GenerateRay without lens effects, the
    primary ray of pixel x through film coordinate (x + sampleOffset) / W, film rows bottom-up"""
    m = np.array(list(camera.localToWorld), dtype=np.float64).reshape(4, 4)
    ys, xs = np.mgrid[0:h, 0:w]
    cx = ((xs + sample_offset[0]) / w) * 2.0 - 1.0
    cy = (((h - 1 - ys) + sample_offset[1]) / h) * 2.0 - 1.0
    direction = (m[0, :3, None, None] * (cx * camera.aspectRatio) + m[1, :3, None, None] * cy) * camera.tanHalfFoV + m[2, :3, None, None]
    return (m[3, :3, None, None] + direction * distance).astype(F)


def test_a_sideways_step_of_one_pixel_is_a_motion_of_one_pixel(built):
    import raytracer_amd as ra
    w, h, distance = 64, 48, 5.0
    vp = ra.Viewport(w, h, seed=3)
    fov = 40.0
    params = {}
    tan_half = np.tan(np.radians(fov) / 2.0)
    pixel = 2.0 * distance * tan_half * (w / h) / w   # a pixel's width at that distance
    for name, x in (("a", 0.0), ("right", pixel), ("left", -pixel)):
        camera = ra.Camera((x, 0.0, 0.0), (0.0, 0.0, 0.0), w / h, fov)
        camera.set_lens(0, 0.0, 0.0)
        params[name] = vp.next_pass_params(camera)
    offsets = {name: tuple(p.sampleOffset) for name, p in params.items()}
    assert any(abs(v) > 1e-3 for v in offsets["a"])   # (the anti-aliasing offset is part of the convention)
    right_axis = np.array(list(params["a"].camera.localToWorld), dtype=np.float64).reshape(4, 4)[0, :3]
    assert abs(right_axis[0]) > 0.99
    plane = lambda name: dict(depth=np.full((h, w), distance, dtype=F), position=unproject(params[name].camera, w, h, offsets["a"], distance),   # (all three with one offset: a difference of offsets is motion too)
                             normal=np.broadcast_to(np.array([0.0, 0.0, -1.0], dtype=F)[:, None, None], (3, h, w)).copy())
    (a0, h0), (a1, h1) = frames(2, w, h)
    first, _, _, _ = ref.accumulate(a0, h0, demodulate=False, **plane("a"))
    for name in ("a", "right", "left"):
        second, motion, taken, why = ref.accumulate(a1, h1, demodulate=False, history=first, prev_world_to_screen=list(params["a"].camera.worldToScreen),
                                                    prev_sample_offset=offsets["a"], **plane(name))
        step = {"a": 0.0, "right": 1.0, "left": -1.0}[name] * np.sign(right_axis[0])
        inner = np.zeros((h, w), dtype=bool)
        inner[2:-2, 2:-2] = True
        assert (why[inner] == ref.BLENDED).all(), name
        assert np.abs(motion[0][inner] - step).max() < 0.01 and np.abs(motion[1][inner]).max() < 0.01, (name, motion[0][inner].mean(), motion[1][inner].mean())


# ---- 4. the variance claim ------------------------------------------------------------------------------------------------------------------------------
def test_the_accumulated_pair_estimates_the_variance_of_the_accumulated_mean():
    """16 frames of independent Gaussian noise around a constant over 4096 pixels: the accumulated error lum(A) - lum(B) is sum w_i e_i with the frames'
    e_i = lum(a_i) - lum(b_i) independent and of zero mean, so the mean of its square is sum w_i^2 Var(e_i).  The estimator's own relative deviation over 4096
    pixels is sqrt(2 / 4096) = 2.2 %: 10 % is four and a half of those."""
    w, h, count, sigma = 64, 64, 16, 0.5
    guides, matrix = flat(w, h)
    sequence = frames(count, w, h, seed=11, sigma=sigma)
    alpha_min, max_history = 0.1, 64.0
    # the blend weights: frame i enters with alpha_i = max(1 / (i + 1), alphaMin) and is scaled by 1 - alpha_j by every later frame j
    alphas = [max(1.0 / (i + 1), alpha_min) for i in range(count)]
    weights = [alphas[i] * np.prod([1.0 - alphas[j] for j in range(i + 1, count)]) for i in range(count)]
    assert abs(sum(weights) - 1.0) < 1e-12
    # per frame e = lum(a) - lum(b) = -lum(noise added to b): the three channels weigh (1, 2, 1) / 4, so Var(e) = sigma^2 * (1 + 4 + 1) / 16
    var_e = sigma * sigma * 6.0 / 16.0
    expected = sum(wt * wt for wt in weights) * var_e
    for history, _, _, _ in run(sequence, guides, matrix, alpha_min=alpha_min, max_history=max_history):
        pass
    e = lum([history["a"][..., k] for k in range(3)]) - lum([history["b"][..., k] for k in range(3)])
    measured = float(np.mean(e.astype(np.float64) ** 2))
    assert abs(measured / expected - 1.0) < 0.10, (measured, expected)
    assert np.array_equal(history["length"], np.full((h, w), float(count), dtype=F))


# ---- 4b. the filter model with the prepare step skipped -----------------------------------------------------------------------------------------------------
def test_the_prepared_filter_model_is_the_existing_one_without_its_prepare_step():
    """colorScale 1 and no demodulation make the existing prepare step c = color * 1, b = colorHalf * 2: exact operations, so the existing model on
    (color, colorHalf) and the prepared one on (color, 2 * colorHalf) must agree to the bit; demodulated, the prepared one on the divided pair"""
    import denoise_var_ref
    f = denoise_var_ref.random_frame_var(37, 23, seed=1000 * 37 + 23)
    guides = dict(depth=f["depth"], normal=f["normal"], position=f["position"])
    for iterations in (1, 3):
        want, want_v = denoise_var_ref.atrous_var(f["color"], f["color_half"], iterations=iterations, demodulate=False, **guides)
        got, got_v = ref.atrous_var_prepared(f["color"], f["color_half"] * F(2.0), iterations=iterations, demodulate=False, **guides)
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)) and np.array_equal(got_v.view(np.uint32), want_v.view(np.uint32))
        want, want_v = denoise_var_ref.atrous_var(f["color"], f["color_half"], albedo=f["albedo"], iterations=iterations, demodulate=True, color_scale=0.25, **guides)
        d = np.moveaxis(np.where(f["albedo"] > F(1e-3), f["albedo"], F(1.0)), 0, -1)
        got, got_v = ref.atrous_var_prepared((f["color"] * F(0.25)) / d, (f["color_half"] * (F(2.0) * F(0.25))) / d, albedo=f["albedo"], iterations=iterations, demodulate=True,
                                             **guides)
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)) and np.array_equal(got_v.view(np.uint32), want_v.view(np.uint32))


# ---- 5. what the random frames of the device tests cover ---------------------------------------------------------------------------------------------------
SHAPES = [(1, 1), (70, 1), (3, 200), (37, 23), (130, 70)]


@pytest.mark.parametrize("w, h", SHAPES, ids=["%dx%d" % s for s in SHAPES])
def test_the_random_frames_reach_every_branch(w, h):
    f = ref.random_temporal_frame(w, h, seed=1000 * w + h)
    for ids in (True, False):
        cur, history = dict(f["current"]), dict(f["history"])
        if not ids:
            cur["object_id"] = history["object_id"] = None
        _, motion, taken, why = ref.accumulate(history=history, prev_world_to_screen=f["prev_world_to_screen"], prev_sample_offset=f["prev_sample_offset"], color_scale=0.25, **cur)
        assert ((taken == 0) == (why != ref.BLENDED)).all() and (why != ref.START_NO_HISTORY).all()
        if w * h < 100:
            continue
        assert (taken == 4).mean() >= 0.20, (taken == 4).mean()
        assert ((taken > 0) & (taken < 4)).mean() >= 0.05
        for reason in (ref.START_INVALID, ref.START_OFF_SCREEN, ref.START_NO_TAP):
            assert (why == reason).mean() >= 0.05, (ids, reason, (why == reason).mean())
        assert np.abs(motion[:, why == ref.BLENDED]).max() > 0.5 and ((motion[1] + np.mgrid[0:h, 0:w][0])[why == ref.BLENDED] < 0).any()   # (taps from row -1)
    assert np.isnan(f["current"]["position"]).sum() == (1 if w * h >= 16 else 0)
