"""tests/temporal_clip_ref.py -- the NumPy float32 model of history clipping (include/rtgpu.h: "Clipping the history", rtgpu_temporal_accumulate_clip) -- held to
the properties it is meant to have.  No GPU: the device is held to the model bit for bit in tests/test_gpu_temporal_clip.py."""
import os

import numpy as np
import pytest

import temporal_clip_ref as cref
import temporal_moving_ref as mref
import temporal_ref as ref

F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(autouse=True, scope="module")
def the_header_defines_what_the_model_restates():
    """the model is the text of a section of include/rtgpu.h: without that section, its entries and its parameter block there is nothing for it to be held to"""
    text = open(os.path.join(ROOT, "include", "rtgpu.h")).read()
    assert "tests/temporal_clip_ref.py" in text and "typedef struct RtTemporalClip" in text
    for entry in ("rtgpu_temporal_accumulate_clip", "rtgpu_temporal_accumulate_clip_async", "rtgpu_denoise_temporal_clip", "rtgpu_denoise_temporal_clip_async"):
        assert "int %s(" % entry in text, entry
    # the ranges the model asserts are the header's
    assert "1, 2 or 3" in text and "[0, 1e6]" in text and "1 .. 49" in text


def words(a):
    return np.ascontiguousarray(a).view(np.uint32)


def same_history(got, want, what):
    for key in ("a", "b", "length", "depth", "normal", "position", "object_id"):
        assert np.array_equal(words(got[key]), words(want[key])), (what, key)


# ---- where nothing clips the model is the existing one, word for word -----------------------------------------------------------------------------------
@pytest.mark.parametrize("demodulate", [True, False], ids=["demodulated", "plain"])
@pytest.mark.parametrize("w, h, seed", [(37, 23, 3), (67, 29, 4)])
def test_a_box_nothing_reaches_is_the_moving_call_word_for_word(w, h, seed, demodulate):
    frame = mref.random_moving_frame(w, h, seed)
    cur = frame["current"]
    kw = dict(color=cur["color"], color_half=cur["color_half"], depth=cur["depth"], normal=cur["normal"], position=cur["position"], albedo=cur["albedo"],
              object_id=cur["object_id"], history=frame["history"], prev_world_to_screen=frame["prev_world_to_screen"], prev_sample_offset=frame["prev_sample_offset"],
              object_motion=frame["object_motion"], demodulate=demodulate)
    want = mref.accumulate_moving(**kw)
    got = cref.accumulate_clip(clip=dict(radius=3, gamma=1e4, min_count=2), **kw)
    info = got[4]
    assert not info["clipped"].any()                       # the condition itself: an input that clips here is the wrong input
    assert (info["f"] == F(1.0)).all()
    blended = want[3] == ref.BLENDED
    assert (blended & (info["cnt"] >= 2)).mean() > 0.2     # ... and the box was there to be reached: pixels that blend, with a window on their surface
    same_history(got[0], want[0], "gamma 1e4")
    assert np.array_equal(words(got[1]), words(want[1])) and np.array_equal(got[2], want[2]) and np.array_equal(got[3], want[3])
    # the restated project / taps / blend alone: no clip at all
    none = cref.accumulate_clip(clip=None, **kw)
    same_history(none[0], want[0], "no clip")
    assert np.array_equal(words(none[1]), words(want[1])) and np.array_equal(none[2], want[2]) and np.array_equal(none[3], want[3])


@pytest.mark.parametrize("ids", [True, False], ids=["ids", "no ids"])
def test_without_a_motion_table_it_is_the_static_call_word_for_word(ids):
    base = ref.random_temporal_frame(37, 23, 5)
    cur = dict(base["current"])
    history = dict(base["history"])
    if not ids:
        cur["object_id"], history["object_id"] = None, None
    kw = dict(cur, history=history, prev_world_to_screen=base["prev_world_to_screen"], prev_sample_offset=base["prev_sample_offset"])
    want = ref.accumulate(**kw)
    for clip in (None, dict(radius=2, gamma=1e4, min_count=2)):
        got = cref.accumulate_clip(clip=clip, **kw)
        assert not got[4]["clipped"].any()
        for key in ("a", "b", "length"):
            assert np.array_equal(words(got[0][key]), words(want[0][key])), (clip, key)
        assert np.array_equal(words(got[1]), words(want[1])) and np.array_equal(got[2], want[2]) and np.array_equal(got[3], want[3])
    # no history: every pixel starts, f = 1
    started = cref.accumulate_clip(clip=dict(radius=1, gamma=0.0, min_count=1), **cur)
    assert (started[0]["length"] == 1.0).all() and (started[4]["f"] == 1.0).all() and not started[4]["clipped"].any()


# ---- a history the light has left ----------------------------------------------------------------------------------------------------------------------------
W, H = 24, 16


def flat_frame(seed=17, object_id=None):
    """a flat, fully valid frame facing the camera, reprojected onto itself: prepared colours 0.05 * (1 +- 0.2), a history of A = B = 1000 of length 32"""
    rng = np.random.default_rng(seed)
    ys, xs = np.mgrid[0:H, 0:W]
    color = (F(0.05) * (F(1.0) + F(0.2) * (rng.random((H, W, 3), dtype=F) * F(2.0) - F(1.0)))).astype(F)
    normal = np.zeros((3, H, W), dtype=F)
    normal[2] = 1.0
    guides = dict(depth=np.full((H, W), 2.0, dtype=F), normal=normal, position=np.stack([xs, ys, np.full((H, W), 2.0)]).astype(F))
    history = dict(guides, a=np.full((H, W, 3), 1000.0, dtype=F), b=np.full((H, W, 3), 1000.0, dtype=F), length=np.full((H, W), 32.0, dtype=F), object_id=object_id)
    return dict(color=color, color_half=(color * F(0.5)).astype(F), albedo=None, demodulate=False, object_id=object_id, history=history,
                prev_world_to_screen=ref.affine_world_to_screen(W, H, (0.0, 0.0)), **guides)


def test_a_history_far_outside_this_frame_s_colours_is_pulled_in_and_forgotten():
    kw = flat_frame()
    clip = dict(radius=3, gamma=2.0, min_count=9)
    got, _, _, why, info = cref.accumulate_clip(clip=clip, **kw)
    assert (why == ref.BLENDED).all()
    assert info["clipped"].all()
    assert (info["cnt"] >= 16).all() and (info["cnt"][3:-3, 3:-3] == 49).all()       # a corner's window holds 4 x 4, the interior's all 49
    assert (got["length"] < 2.0).all()
    c = [kw["color"][..., k] for k in range(3)]
    mu, g, _ = cref.moments(c, kw["depth"], kw["normal"], kw["position"], None, 3, 2.0)
    for k in range(3):
        bound = np.maximum(c[k], mu[k] + g[k]).astype(np.float64) * (1.0 + 1e-6)
        assert (got["a"][..., k] <= bound).all(), k
        assert (np.abs(mu[k] - 0.05) < 0.01).all() and (g[k] > 0.0).all() and (g[k] < 0.02).all()    # the box is this frame's: around 0.05, two sigma of a uniform +-0.01
    assert (info["f"] < 1e-3).all() and (info["f"] > 0.0).all()
    unclipped = cref.accumulate_clip(clip=None, **kw)[0]
    assert (unclipped["a"] > 900.0).all()
    assert (ref.accumulate(**kw)[0]["a"] > 900.0).all()


def test_a_pixel_with_too_little_of_its_surface_in_the_window_is_the_unclipped_call_s():
    """a one-pixel object id island: its window holds one pixel of its surface -- itself -- and min_count asks for more"""
    ids = np.zeros((H, W), dtype=np.uint32)
    island = (8, 12)
    ids[island] = 5
    kw = flat_frame(object_id=ids)
    unclipped = cref.accumulate_clip(clip=None, **kw)
    for min_count in (2, 9):
        got = cref.accumulate_clip(clip=dict(radius=3, gamma=2.0, min_count=min_count), **kw)
        info = got[4]
        assert got[3][island] == ref.BLENDED and unclipped[3][island] == ref.BLENDED
        assert info["cnt"][island] == 1.0 and not info["clipped"][island] and info["f"][island] == 1.0
        for key in ("a", "b", "length"):
            assert np.array_equal(words(got[0][key][island]), words(unclipped[0][key][island])), key
        assert got[0]["a"][island].min() > 900.0
        everyone_else = np.ones((H, W), dtype=bool)
        everyone_else[island] = False
        assert info["clipped"][everyone_else].all() and (got[0]["length"][everyone_else] < 2.0).all()
    # with min_count = 1 the island clips to its own colour: a box of no width
    alone = cref.accumulate_clip(clip=dict(radius=3, gamma=2.0, min_count=1), **kw)
    assert alone[4]["clipped"][island] and alone[4]["f"][island] == 0.0 and alone[0]["length"][island] == 1.0
    assert np.array_equal(words(alone[0]["a"][island]), words(kw["color"][island]))


def test_b_is_shifted_by_what_a_was_pulled():
    """Every value a power of two or a small integer, so that nothing rounds: pixels paired by their ids, each pair's colours 1 and 3 -- mu = 2, var = 10 / 2 - 4 = 1,
    g = 1, the box [1, 3]; the history A = 64, B = 96 of length 2^30 under alpha_min = 0.5, so that alpha is 0.5 clipped or not.  A is pulled to 3 and B goes along
    to 35: outB' - outA' = 0.5 * (35 - 3) is the unclipped 0.5 * (96 - 64)."""
    ys, xs = np.mgrid[0:H, 0:W]
    ids = (ys * (W // 2) + xs // 2).astype(np.uint32)
    kw = flat_frame(object_id=ids)
    color = np.where((xs % 2 == 0)[..., None], F(1.0), F(3.0)) * np.ones((H, W, 3), dtype=F)
    kw.update(color=color.astype(F), color_half=(color * F(0.5)).astype(F), alpha_min=0.5)
    kw["history"] = dict(kw["history"], a=np.full((H, W, 3), 64.0, dtype=F), b=np.full((H, W, 3), 96.0, dtype=F), length=np.full((H, W), 2.0 ** 30, dtype=F))
    clipped, _, _, why, info = cref.accumulate_clip(clip=dict(radius=1, gamma=1.0, min_count=2), **kw)
    unclipped = cref.accumulate_clip(clip=None, **kw)[0]
    assert (why == ref.BLENDED).all() and (info["cnt"] == 2.0).all() and info["clipped"].all()
    assert (info["f"] == F(3.0) / (F(3.0) + F(183.0))).all()
    assert (clipped["length"] == 64.0).all() and (unclipped["length"] == 64.0).all()
    c = color.astype(F)
    assert np.array_equal(clipped["a"], (F(3.0) + F(0.5) * (c - F(3.0))).astype(F)) and np.array_equal(clipped["b"], (F(35.0) + F(0.5) * (c - F(35.0))).astype(F))
    assert np.array_equal(words(clipped["b"] - clipped["a"]), words(unclipped["b"] - unclipped["a"]))
    assert (clipped["b"] - clipped["a"] == 16.0).all()


def test_the_moments_of_a_window():
    """against float64 statistics of the same window, on a frame with an id edge and a miss"""
    rng = np.random.default_rng(2)
    kw = flat_frame()
    ids = np.zeros((H, W), dtype=np.uint32)
    ids[:, W // 2:] = 1
    depth = kw["depth"].copy()
    depth[4, 5] = np.inf
    c = [kw["color"][..., k] * F(rng.uniform(0.5, 2.0)) for k in range(3)]
    for radius in (1, 2, 3):
        mu, g, cnt = cref.moments(c, depth, kw["normal"], kw["position"], ids, radius, 1.5)
        for (y, x) in ((0, 0), (4, 4), (7, W // 2 - 1), (7, W // 2), (H - 1, W - 1)):
            ys, xs = np.mgrid[max(0, y - radius):min(H, y + radius + 1), max(0, x - radius):min(W, x + radius + 1)]
            keep = (ids[ys, xs] == ids[y, x]) & np.isfinite(depth[ys, xs])
            assert cnt[y, x] == keep.sum()
            for k in range(3):
                values = c[k][ys, xs][keep].astype(np.float64)
                assert abs(mu[k][y, x] - values.mean()) < 1e-6 and abs(g[k][y, x] - 1.5 * values.std()) < 1e-4
