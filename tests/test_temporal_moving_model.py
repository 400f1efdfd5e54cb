"""tests/temporal_moving_ref.py -- the NumPy float32 model of temporal accumulation that follows moving objects (include/rtgpu.h:
rtgpu_temporal_accumulate_moving) and the double-precision motion-table builder -- held to the properties they are meant to have.  No GPU: the device is
held to the model bit for bit in tests/test_gpu_temporal_moving.py."""
import numpy as np
import pytest

import temporal_moving_ref as mref
import temporal_ref as ref

F = np.float32


def words(a):
    return np.ascontiguousarray(a).view(np.uint32)


def run(frame, **extra):
    cur = frame["current"]
    return mref.accumulate_moving(cur["color"], cur["color_half"], cur["depth"], cur["normal"], cur["position"], cur["albedo"], cur["object_id"], frame["history"],
                                  frame["prev_world_to_screen"], frame["prev_sample_offset"], object_motion=frame["object_motion"], **extra)


@pytest.mark.parametrize("seed", [3, 4])
def test_a_table_of_unmoved_objects_is_the_static_call_word_for_word(seed):
    """moved = 0 everywhere and prev ids that are the ids: the select keeps every position and normal, and the results are temporal_ref.accumulate's -- with
    matrices full of rubbish, which nobody may read a value from"""
    base = ref.random_temporal_frame(37, 23, seed)
    cur = base["current"]
    n = int(max(cur["object_id"].max(), base["history"]["object_id"].max())) + 1
    rubbish = np.random.default_rng(seed).normal(size=(n, 4, 4)).astype(F)
    rubbish[0, 0, 0] = np.nan
    table = (rubbish, np.arange(n, dtype=np.uint32), np.zeros(n, dtype=np.uint32))
    for demodulate in (True, False):
        want = ref.accumulate(cur["color"], cur["color_half"], cur["depth"], cur["normal"], cur["position"], cur["albedo"], cur["object_id"], base["history"],
                              base["prev_world_to_screen"], base["prev_sample_offset"], demodulate=demodulate)
        got = mref.accumulate_moving(cur["color"], cur["color_half"], cur["depth"], cur["normal"], cur["position"], cur["albedo"], cur["object_id"], base["history"],
                                     base["prev_world_to_screen"], base["prev_sample_offset"], object_motion=table, demodulate=demodulate)
        for key in ("a", "b", "length", "depth", "normal", "position", "object_id"):
            assert np.array_equal(words(got[0][key]), words(want[0][key]), ), key
        assert np.array_equal(words(got[1]), words(want[1])) and np.array_equal(got[2], want[2]) and np.array_equal(got[3], want[3])
        assert (want[3] == ref.BLENDED).mean() > 0.3


@pytest.mark.parametrize("seed,num_objects", [(11, 3), (12, 4), (13, 5)])
def test_random_frames_cover_every_way_a_tap_drops_out(seed, num_objects):
    frame = mref.random_moving_frame(130, 70, seed, num_objects)
    history, motion, taken, reason = run(frame)
    planted, cur = frame["planted"], frame["current"]
    matrices, prev_ids, moved = frame["object_motion"]
    # 3 .. 5 objects under distinct rigid motions, a permuted id space
    assert len(prev_ids) == num_objects and sorted(prev_ids.tolist()) == list(range(num_objects)) and not np.array_equal(prev_ids, np.arange(num_objects))
    assert moved.tolist() == [0] + [1] * (num_objects - 1)
    assert len({m.tobytes() for m in matrices}) == num_objects
    for m in matrices:      # rigid: the rotation part is orthonormal
        assert np.abs(m[:3, :3].astype(np.float64) @ m[:3, :3].astype(np.float64).T - np.eye(3)).max() < 1e-6
    moving = planted["moving"]
    assert moving.sum() > 0.5 * moving.size
    blended = reason == ref.BLENDED
    assert blended[moving].mean() >= 0.30 and (~blended)[moving].mean() >= 0.15
    # every object's pixels accumulate somewhere: the matrix brings them back onto the history
    for o in range(num_objects):
        mine = (cur["object_id"] == o)
        assert mine.any() and blended[mine].mean() > 0.3, o
    # id: a pixel that claims the neighbouring object lands on the history (its geometry matches) and is refused by the id it had then -- unless it sits on
    # the border of that very neighbour's block, where a tap may carry the id it claims
    base_reason = ref.accumulate(**{k: v for k, v in frame["base"]["current"].items() if k != "object_id"}, history=dict(frame["base"]["history"], object_id=None),
                                 prev_world_to_screen=frame["prev_world_to_screen"], prev_sample_offset=frame["prev_sample_offset"])[3]
    claims = planted["claims_neighbour"] & (base_reason == ref.BLENDED)       # (pixels the geometry alone would accumulate)
    assert claims.sum() > 20 and (reason[claims] == ref.START_NO_TAP).mean() > 0.8
    # ... and a history pixel of an id no object had drops out of its neighbours' taps: pixels that took one to three
    assert planted["stranger"].sum() > 20 and ((taken > 0) & (taken < 4)).sum() > 20
    # out-of-range id: starts, as a miss does (the table is not read: the model indexes record 0 and drops it)
    outside = planted["outside_table"]
    assert outside.sum() > 20 and (reason[outside] == ref.START_INVALID).all() and (history["length"][outside] == 1.0).all()
    # normal, plane, off-frame: what the base frame plants (temporal_ref.random_temporal_frame), seen through the motion
    for why in (ref.START_OFF_SCREEN, ref.START_NO_TAP):
        assert ((reason == why) & (base_reason == why) & moving).sum() > 20, why
    base_cur = frame["base"]["current"]
    turned = (np.abs(base_cur["normal"][0]) > 0.9) & moving
    lifted = (base_cur["position"][2] > 2.5) & moving
    assert turned.sum() > 20 and (reason[turned] != ref.BLENDED).all() and lifted.sum() > 20 and (reason[lifted] != ref.BLENDED).all()
    # the stored history keeps the CURRENT guides
    for key in ("normal", "position", "object_id", "depth"):
        assert np.array_equal(words(history[key]), words(cur[key])), key


def test_the_motion_brings_a_moved_surface_back_exactly_where_rounding_allows():
    """a flat surface carried along by one object: every interior pixel takes all four taps and the motion plane shows the camera's shift alone"""
    w, h = 32, 16
    ys, xs = np.mgrid[0:h, 0:w]
    rng = np.random.default_rng(5)
    motion = mref.rigid(rng)
    then = np.stack([xs, ys, np.full((h, w), 2.0)]).astype(np.float64)
    now = (np.concatenate([then.reshape(3, -1), np.ones((1, w * h))]).T @ np.linalg.inv(motion))[:, :3].T.reshape(3, h, w)
    normal_now = (np.array([0.0, 0.0, 1.0]) @ np.linalg.inv(motion)[:3, :3])
    guides = dict(depth=np.full((h, w), 2.0, dtype=F), normal=np.broadcast_to(normal_now[:, None, None], (3, h, w)).astype(F), position=now.astype(F))
    previous = dict(depth=guides["depth"], normal=np.broadcast_to(np.array([0.0, 0.0, 1.0], dtype=F)[:, None, None], (3, h, w)).copy(), position=then.astype(F),
                    object_id=np.full((h, w), 4, dtype=np.uint32), a=np.full((h, w, 3), 3.0, dtype=F), b=np.full((h, w, 3), 3.0, dtype=F), length=np.full((h, w), 5.0, dtype=F))
    color = np.ones((h, w, 3), dtype=F)
    table = (np.stack([np.eye(4), motion]).astype(F), np.array([9, 4], dtype=np.uint32), np.array([0, 1], dtype=np.uint32))
    history, moved_by, taken, reason = mref.accumulate_moving(color, color * F(0.5), albedo=None, demodulate=False, object_id=np.ones((h, w), dtype=np.uint32), history=previous,
                                                              prev_world_to_screen=ref.affine_world_to_screen(w, h, (0.5, 0.25)), object_motion=table, **guides)
    assert (reason == ref.BLENDED).all() and (taken[:-1, :-1] == 4).all()
    assert np.abs(moved_by[0] - 0.5).max() < 1e-4 and np.abs(moved_by[1] - 0.25).max() < 1e-4
    assert (history["length"] == 6.0).all() and np.abs(history["a"] - (3.0 + (1.0 - 3.0) / 6.0)).max() < 1e-5
    # the same pixels under the static definition: the surface is somewhere else, nothing is found
    static = ref.accumulate(color, color * F(0.5), albedo=None, demodulate=False, object_id=np.full((h, w), 4, dtype=np.uint32), history=previous,
                            prev_world_to_screen=ref.affine_world_to_screen(w, h, (0.5, 0.25)), **guides)
    assert (static[3] != ref.BLENDED).mean() > 0.9


def test_the_table_builder():
    rng = np.random.default_rng(9)
    n = 6
    then = np.stack([mref.rigid(rng) for _ in range(n)]).astype(F)
    now = then.copy()
    now[1::2] = np.stack([mref.rigid(rng) for _ in range(n // 2)]).astype(F)
    inverse = np.stack([np.linalg.inv(m.astype(np.float64)) for m in now]).astype(F)
    ids = rng.permutation(n).astype(np.uint32)
    matrices, prev_ids, moved = mref.motion_table(now, inverse, then, ids)
    assert matrices.dtype == F and matrices.shape == (n, 4, 4) and np.array_equal(prev_ids, ids)
    assert moved.tolist() == [0, 1] * (n // 2)
    # the float64 product, whichever way it is summed, rounds to the same floats or their neighbours; the stated order is the definition
    assert np.abs(matrices - (inverse.astype(np.float64) @ then.astype(np.float64))).max() < 1e-6
    for o in range(n):
        for i in range(4):
            for j in range(4):
                s = float(inverse[o, i, 0]) * float(then[o, 0, j])
                for k in range(1, 4):
                    s = s + float(inverse[o, i, k]) * float(then[o, k, j])
                assert matrices[o, i, j] == F(s)
    # an unmoved object's matrix is the identity up to the inverse's rounding -- and nobody reads it: moved = 0 selects the pixel's own position
    assert np.abs(matrices[0] - np.eye(4)).max() < 1e-5
    # a bit flipped in the transform is a move
    nudged = now.copy()
    nudged.view(np.uint32)[0, 3, 1] ^= 1
    assert mref.motion_table(nudged, inverse, then, ids)[2][0] == 1
