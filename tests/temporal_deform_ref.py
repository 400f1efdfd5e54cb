"""Temporal accumulation that follows deforming meshes (include/rtgpu.h: rtgpu_temporal_accumulate_deform) as a NumPy float32 model, and the builder of the
table rtgpu_denoise_temporal builds under rtgpu_set_deform_tracking.  The device is held to both bit for bit (tests/test_gpu_temporal_deform.py); the model's
own properties: tests/test_temporal_deform_model.py.

The definition restates one thing of the moving call and leaves the rest alone, and so does the model: where_it_was is temporal_moving_ref.where_it_was with,
for the pixels of a record marked RT_MOTION_DEFORMED, the point taken from the old triangle record and the normal left as it is.  Everything behind that step
-- project, taps, clip, blend -- is temporal_clip_ref.accumulate_clip, which calls the step by name: accumulate_deform lends it this module's for one call."""
import numpy as np

import temporal_clip_ref
import temporal_moving_ref
from temporal_ref import F

RT_MOTION_DEFORMED = 2
_moving_step = temporal_moving_ref.where_it_was      # (the moving rules' own step, whatever accumulate_deform lends the module meanwhile)


def where_it_was(normal, position, object_id, object_motion, deform):
    """(N', P', the id then, known): the per-pixel step of the definition.  deform = dict(sub_object_id (H, W) uint32, barycentrics (2, H, W) float32,
    prev_triangles (T, 9) float32, first_triangle (n,), num_triangles (n,))"""
    matrices, prev_ids, moved = object_motion
    matrices = np.ascontiguousarray(matrices, dtype=F).reshape(-1, 4, 4)
    moved = np.asarray(moved).reshape(-1)
    assert (moved <= RT_MOTION_DEFORMED).all()
    n = matrices.shape[0]
    h, w = normal.shape[1:]
    # records 0 and 1: the moving rules (a deformed record goes through them as one that stood still, and is overwritten below)
    n_then, p_then, id_then, known = _moving_step(normal, position, object_id, (matrices, prev_ids, np.where(moved == RT_MOTION_DEFORMED, 0, moved)))
    ids = np.asarray(object_id, dtype=np.uint32).reshape(h, w)
    o = np.where(ids < n, ids, 0).astype(np.int64)
    deformed = known & (moved[o] == RT_MOTION_DEFORMED)
    triangles = np.ascontiguousarray(deform["prev_triangles"], dtype=F).reshape(-1, 9)
    first = np.asarray(deform["first_triangle"]).reshape(-1).astype(np.int64)[o]      # (no 32-bit wrap-around: int64)
    count = np.asarray(deform["num_triangles"]).reshape(-1).astype(np.int64)[o]
    t = np.asarray(deform["sub_object_id"], dtype=np.uint32).reshape(h, w).astype(np.int64)
    u, v = np.asarray(deform["barycentrics"], dtype=F).reshape(2, h, w)
    in_range = (t < count) & (first + t < triangles.shape[0])
    follows = deformed & in_range
    record = triangles[np.where(follows, first + t, 0)] if triangles.shape[0] else np.zeros((h, w, 9), dtype=F)      # (never read out of range)
    m = matrices[o]
    with np.errstate(all="ignore"):
        local = []
        for k in range(3):
            lk = record[..., 3 + k] * u + record[..., k]
            lk = record[..., 6 + k] * v + lk
            local.append(lk.astype(F))
        for j in range(3):
            pj = local[0] * m[..., 0, j] + m[..., 3, j]
            pj = local[1] * m[..., 1, j] + pj
            pj = local[2] * m[..., 2, j] + pj
            p_then[j] = np.where(follows, pj, p_then[j]).astype(F)
            n_then[j] = np.where(deformed, normal[j], n_then[j]).astype(F)          # N' = N_p
    return n_then, p_then, id_then, known & (~deformed | in_range)


def accumulate_deform(color, color_half, depth, normal, position, albedo=None, object_id=None, history=None, prev_world_to_screen=None, prev_sample_offset=(0.0, 0.0),
                      object_motion=None, deform=None, clip=None, **params):
    """temporal_clip_ref.accumulate_clip's arguments and results (clip may be None), with deform as where_it_was takes it and an object_motion whose moved may hold
    RT_MOTION_DEFORMED"""
    assert object_motion is not None and deform is not None
    temporal_moving_ref.where_it_was = lambda n, p, i, table: where_it_was(n, p, i, table, deform)
    try:
        return temporal_clip_ref.accumulate_clip(color, color_half, depth, normal, position, albedo, object_id, history, prev_world_to_screen, prev_sample_offset,
                                                 object_motion=object_motion, clip=clip, **params)
    finally:
        temporal_moving_ref.where_it_was = _moving_step


def context_table(transform_now, inverse_now, transform_then, id_then, deformed, first_triangle, num_triangles):
    """The table rtgpu_denoise_temporal[_clip] builds: temporal_moving_ref.motion_table's, and for every object of `deformed` (a bool per object) moved =
    RT_MOTION_DEFORMED and m = the words of the transform it had then.  Returns (object_motion, first_triangle (n,), num_triangles (n,)): the last two are the
    object's mesh's range for a deformed object, 0 for the others."""
    matrices, prev_ids, moved = temporal_moving_ref.motion_table(transform_now, inverse_now, transform_then, id_then)
    deformed = np.asarray(deformed, dtype=bool).reshape(-1)
    then = np.ascontiguousarray(transform_then, dtype=F).reshape(-1, 4, 4)
    matrices = np.where(deformed[:, None, None], then, matrices).astype(F)
    moved = np.where(deformed, RT_MOTION_DEFORMED, moved).astype(np.uint32)
    first = np.where(deformed, np.asarray(first_triangle).reshape(-1), 0).astype(np.uint32)
    count = np.where(deformed, np.asarray(num_triangles).reshape(-1), 0).astype(np.uint32)
    return (matrices, prev_ids, moved), first, count


LEADING, TRAILING = 5, 3      # records of other meshes around the deformed one's in the random frame's triangle table: nobody may read a value from them


def random_deform_frame(w, h, seed, num_objects=4):
    """temporal_moving_ref.random_moving_frame with its last object turned into a deformed mesh: its record is RT_MOTION_DEFORMED with a random rigid transform
    of then; a small table of large triangles tiles the plane the history lies in, in that transform's local space, and each of the object's pixels carries the
    triangle and the barycentrics of where its surface point was.  Its current position is thrown somewhere else -- the definition does not read it -- and its
    normal is the one it had (N' = N_p).  Planted: triangle ids past the mesh's count, and 0xFFFFFFFF.  Returns the frame plus `deform` and, in `planted`,
    `deformed` (the object's valid pixels) and `bad_triangle`."""
    frame = temporal_moving_ref.random_moving_frame(w, h, seed, num_objects)
    rng = np.random.default_rng(seed + 104729)
    cur, base = dict(frame["current"]), frame["base"]["current"]
    matrices, prev_ids, moved = (a.copy() for a in frame["object_motion"])
    d = num_objects - 1
    mine = (cur["object_id"] == d) & np.isfinite(cur["depth"])
    then = temporal_moving_ref.rigid(rng)                      # local then -> world then (row vectors)
    matrices[d], moved[d] = then.astype(F), RT_MOTION_DEFORMED
    # the plane z = 2.0005 of the world of then, over the frame and a margin, in cells of two triangles
    cells_x, cells_y, margin = 4, 3, 3.0
    gx, gy = np.linspace(-margin, w + margin, cells_x + 1), np.linspace(-margin, h + margin, cells_y + 1)
    corners = np.array([[[gx[i], gy[j], 2.0005, 1.0] for i in range(cells_x + 1)] for j in range(cells_y + 1)]) @ np.linalg.inv(then.astype(F).astype(np.float64))
    records = []
    for j in range(cells_y):
        for i in range(cells_x):
            a, b, c, e = corners[j, i, :3], corners[j, i + 1, :3], corners[j + 1, i + 1, :3], corners[j + 1, i, :3]
            records += [np.concatenate([a, b - a, c - a]), np.concatenate([a, c - a, e - a])]
    num = len(records)
    table = np.full((LEADING + num + TRAILING, 9), np.nan, dtype=F)
    table[LEADING:LEADING + num] = np.array(records).astype(F)
    # where each pixel's surface point was: the base frame's position; its cell, its triangle of the two, its barycentrics there (in the world of then, in double)
    was = np.where(np.isfinite(base["position"]), base["position"], 0.0).astype(np.float64)      # (the base frame's one NaN position: masked out by `ok`)
    ci = np.clip(((was[0] + margin) / (gx[1] - gx[0])).astype(np.int64), 0, cells_x - 1)
    cj = np.clip(((was[1] + margin) / (gy[1] - gy[0])).astype(np.int64), 0, cells_y - 1)
    fx, fy = (was[0] - gx[ci]) / (gx[1] - gx[0]), (was[1] - gy[cj]) / (gy[1] - gy[0])
    lower = fx >= fy                                            # a, b, c: P = a + (fx - fy) (b - a) + fy (c - a);  a, c, e: P = a + fx (c - a) + (fy - fx) (e - a)
    sub = (2 * (cj * cells_x + ci) + np.where(lower, 0, 1)).astype(np.uint32)
    bary = np.stack([np.where(lower, fx - fy, fx), np.where(lower, fy, fy - fx)])
    ok = mine & np.isfinite(base["position"]).all(axis=0)
    sub = np.where(ok, sub, rng.integers(0, 1 << 20, size=(h, w))).astype(np.uint32)          # (rubbish off the mesh: not read)
    bary = np.where(ok, bary, 0.0).astype(F)
    bad = mine & (rng.random((h, w)) < 0.05) & (w * h >= 16)
    sub[bad] = np.where(rng.random(int(bad.sum())) < 0.5, num + rng.integers(0, TRAILING + 2, size=int(bad.sum())), 0xFFFFFFFF).astype(np.uint32)
    position, normal = cur["position"].copy(), cur["normal"].copy()
    position[:, mine] = (position[:, mine] + rng.normal(scale=5.0, size=(3, int(mine.sum())))).astype(F)
    normal[:, mine] = base["normal"][:, mine]
    cur.update(position=position, normal=normal)
    n = len(moved)
    deform = dict(sub_object_id=sub, barycentrics=bary, prev_triangles=table, first_triangle=np.where(np.arange(n) == d, LEADING, 0).astype(np.uint32),
                  num_triangles=np.where(np.arange(n) == d, num, 0).astype(np.uint32))
    return dict(frame, current=cur, object_motion=(matrices, prev_ids, moved), deform=deform, planted=dict(frame["planted"], deformed=mine, bad_triangle=bad, object=d))
