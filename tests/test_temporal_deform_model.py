"""tests/temporal_deform_ref.py -- the NumPy float32 model of temporal accumulation that follows deforming meshes (include/rtgpu.h:
rtgpu_temporal_accumulate_deform) -- held to the properties it is meant to have, and the deformation of the device test held to the one condition that test
puts on its inputs.  No GPU: the device is held to the model bit for bit in tests/test_gpu_temporal_deform.py."""
import numpy as np
import pytest

import temporal_deform_ref as dref
import temporal_moving_ref as mref
import temporal_ref as ref

F = np.float32
KEYS = ("a", "b", "length", "depth", "normal", "position", "object_id")
CLIPS = [None, dict(radius=2, gamma=1.0, min_count=5)]


def words(a):
    return np.ascontiguousarray(a).view(np.uint32)


def run(frame, clip=None, **change):
    cur = frame["current"]
    args = dict(object_motion=frame["object_motion"], deform=frame["deform"])
    args.update(change)
    return dref.accumulate_deform(cur["color"], cur["color_half"], cur["depth"], cur["normal"], cur["position"], cur["albedo"], cur["object_id"], frame["history"],
                                  frame["prev_world_to_screen"], frame["prev_sample_offset"], clip=clip, **args)


def same(got, want, where=None):
    for key in KEYS:
        a, b = words(got[0][key]), words(want[0][key])
        if where is not None:
            a, b = a[..., where, :] if key in ("a", "b") else a[..., where], b[..., where, :] if key in ("a", "b") else b[..., where]
        assert np.array_equal(a, b), key
    pick = (lambda x: x) if where is None else (lambda x: x[..., where])
    assert np.array_equal(pick(words(got[1])), pick(words(want[1]))) and np.array_equal(pick(got[2]), pick(want[2])) and np.array_equal(pick(got[3]), pick(want[3]))


@pytest.mark.parametrize("seed", [3, 4])
def test_without_a_deformed_record_it_is_the_moving_call_word_for_word(seed):
    """the identity of the header: a table of records 0 and 1 -- with planes and a triangle table full of rubbish, which nobody may read a value from"""
    frame = mref.random_moving_frame(37, 23, seed)
    rng = np.random.default_rng(seed)
    n = len(frame["object_motion"][2])
    rubbish = dict(sub_object_id=rng.integers(0, 1 << 32, size=(23, 37)).astype(np.uint32), barycentrics=np.full((2, 23, 37), np.nan, dtype=F),
                   prev_triangles=np.full((4, 9), np.nan, dtype=F), first_triangle=rng.integers(0, 1 << 32, size=n), num_triangles=rng.integers(0, 1 << 32, size=n))
    cur = frame["current"]
    for demodulate in (True, False):
        want = mref.accumulate_moving(cur["color"], cur["color_half"], cur["depth"], cur["normal"], cur["position"], cur["albedo"], cur["object_id"], frame["history"],
                                      frame["prev_world_to_screen"], frame["prev_sample_offset"], object_motion=frame["object_motion"], demodulate=demodulate)
        got = run(dict(frame, deform=rubbish), demodulate=demodulate)
        same(got, want)
        assert (want[3] == ref.BLENDED).mean() > 0.3


@pytest.mark.parametrize("clip", CLIPS, ids=["plain", "clip"])
@pytest.mark.parametrize("seed", [5, 6])
def test_a_deformed_objects_pixels_blend_through_their_old_triangles(seed, clip):
    """the object's pixels carry triangle ids and barycentrics into a small table whose points lie on the history: they blend.  With the same record marked
    0xFFFFFFFF -- the table the context builds without tracking -- exactly those pixels start, and every other pixel is word-equal"""
    frame = dref.random_deform_frame(70, 41, seed)
    planted = frame["planted"]
    d, mine, bad = planted["object"], planted["deformed"], planted["bad_triangle"]
    matrices, prev_ids, moved = frame["object_motion"]
    assert sorted(set(moved.tolist())) == [0, 1, 2] and moved[d] == dref.RT_MOTION_DEFORMED
    got = run(frame, clip)
    blended = got[3] == ref.BLENDED
    good = mine & ~bad
    assert good.sum() > 200 and blended[good].mean() > 0.5
    assert bad.sum() >= 3 and not blended[bad].any() and (got[0]["length"][bad] == 1).all()
    # (the current position of those pixels is thrown metres off: had it been read, nothing would have blended)
    dropped = prev_ids.copy()
    dropped[d] = 0xFFFFFFFF
    want = run(frame, clip, object_motion=(matrices, dropped, np.where(moved == dref.RT_MOTION_DEFORMED, 0, moved)))
    assert not (want[3] == ref.BLENDED)[mine].any() and (want[0]["length"][mine] == 1).all()
    same(got, want, ~mine)
    if clip is not None:
        for key in ("cnt", "f"):
            assert np.array_equal(words(got[4][key])[~mine], words(want[4][key])[~mine])


def test_a_triangle_outside_its_range_starts_the_pixel_and_nothing_else_changes():
    frame = dref.random_deform_frame(37, 23, 8)
    d, mine, bad = frame["planted"]["object"], frame["planted"]["deformed"], frame["planted"]["bad_triangle"]
    base = run(frame)
    blended = (base[3] == ref.BLENDED) & mine & ~bad
    y, x = np.argwhere(blended)[0]
    num = int(frame["deform"]["num_triangles"][d])
    one = np.zeros_like(mine)
    one[y, x] = True
    # an id >= num_triangles (the record behind the mesh's last exists in the table: the count decides)
    for t in (num, num + 1, 0x7FFFFFFF, 0xFFFFFFFF):
        sub = frame["deform"]["sub_object_id"].copy()
        sub[y, x] = t
        got = run(frame, deform=dict(frame["deform"], sub_object_id=sub))
        assert got[3][y, x] == ref.START_INVALID and got[0]["length"][y, x] == 1
        same(got, base, ~one)
    # a range that overruns the table by one: the pixels of the last triangle start, every other pixel is untouched
    table = frame["deform"]["prev_triangles"]
    short = dict(frame["deform"], prev_triangles=table[:dref.LEADING + num - 1].copy())
    last = mine & (frame["deform"]["sub_object_id"] == num - 1)
    assert (last & blended).any()
    got = run(frame, deform=short)
    assert (got[3][last] == ref.START_INVALID).all()
    same(got, base, ~last)
    # first + t past 2^32: no wrap-around into the table
    wrapped = dict(frame["deform"], first_triangle=np.where(np.arange(len(frame["deform"]["first_triangle"])) == d, 0xFFFFFFFF, 0).astype(np.uint32))
    got = run(frame, deform=wrapped)
    assert not (got[3] == ref.BLENDED)[mine].any()
    same(got, base, ~mine)
    # and an empty table
    got = run(frame, deform=dict(frame["deform"], prev_triangles=np.zeros((0, 9), dtype=F)))
    same(got, base, ~mine)


def test_the_context_table_keeps_the_id_and_the_transform_of_then():
    rng = np.random.default_rng(21)
    now = np.stack([mref.rigid(rng) for _ in range(4)]).astype(F)
    then = now.copy()
    then[1], then[2] = mref.rigid(rng).astype(F), mref.rigid(rng).astype(F)
    inverse = np.linalg.inv(now.astype(np.float64)).astype(F)
    (matrices, prev_ids, moved), first, count = dref.context_table(now, inverse, then, [3, 2, 1, 0], [False, False, True, True], [0, 0, 7, 7], [0, 0, 512, 512])
    plain = mref.motion_table(now, inverse, then, [3, 2, 1, 0])
    assert moved.tolist() == [0, 1, 2, 2] and prev_ids.tolist() == [3, 2, 1, 0] and first.tolist() == [0, 0, 7, 7] and count.tolist() == [0, 0, 512, 512]
    assert np.array_equal(words(matrices[:2]), words(plain[0][:2])) and np.array_equal(words(matrices[2:]), words(then[2:]))


# ---- the deformation of tests/test_gpu_temporal_deform.py: the condition that test puts on its inputs, from the oracle's planes ------------------------------
@pytest.mark.parametrize("kind", ["two_level", "single"])
def test_the_device_tests_deformation_lets_more_than_half_of_the_mesh_blend(built, kind):
    """tests/test_gpu_temporal_deform.py must not pass vacuously: of the pixels on the mesh that are valid in both frames more than half blend.  That is a
    property of its deformation, its camera and the defaults -- checked here by the model alone, over first-hit planes the CPU oracle renders"""
    import deform_scenes as ds
    import mesh_refit_scenes as ms
    scene, camera, pos, idx, nrm = ms.SCENES[kind]("grid17", ds.W / ds.H)
    params = ds.guide_params(camera)
    before = ds.oracle_planes(scene, params[0])
    triangles = ds.scene_triangles(scene)
    then = ds.object_tables(scene)
    ds.deform(scene, None, pos, idx, 1)
    after = ds.oracle_planes(scene, params[1])
    table, deform = ds.context_inputs(scene, then, triangles, after)
    ones = np.ones((ds.H, ds.W, 3), dtype=F)
    history = dict(a=ones, b=ones, length=np.ones((ds.H, ds.W), dtype=F), depth=before["depth"], normal=before["normal"], position=before["position"], object_id=before["object_id"])
    got = dref.accumulate_deform(ones, ones, after["depth"], after["normal"], after["position"], None, after["object_id"], history,
                                 list(params[0].camera.worldToScreen), tuple(params[0].sampleOffset), object_motion=table, deform=deform, demodulate=False)
    on_mesh = np.isin(after["object_id"], ds.mesh_objects(scene)) & np.isfinite(after["depth"]) & np.isin(before["object_id"], ds.mesh_objects(scene))
    assert on_mesh.sum() > 300
    assert (got[3] == ref.BLENDED)[on_mesh].mean() > 0.5, (got[3] == ref.BLENDED)[on_mesh].mean()
    # ... and the deformation is one: most of those pixels' surface points moved by more than the plane tolerance allows a static reprojection
    moved = np.abs(got[1][:, on_mesh]).max(axis=0)
    assert (moved > 0.25).mean() > 0.5
