"""Temporal accumulation that follows moving objects (include/rtgpu.h: rtgpu_temporal_accumulate_moving) as a NumPy float32 model, and the double-precision
builder of the motion table rtgpu_denoise_temporal builds from two object tables.  The device is held to both bit for bit
(tests/test_gpu_temporal_moving.py); the model's own properties: tests/test_temporal_moving_model.py.

The definition restates three things of the static call and leaves the rest alone, and so does the model: it computes, per pixel, where the surface point was
in the previous frame (P', N') and which id its object had there, and hands those to temporal_ref.accumulate in place of the pixel's own; a pixel whose id is
outside the table is handed over as a miss (it starts).  What comes back as the next history holds the CURRENT normal, position and ids."""
import numpy as np

import temporal_ref
from temporal_ref import F

RT_INVALID_OBJECT = 0xFFFFFFFF


def motion_table(transform_now, inverse_now, transform_then, id_then):
    """(matrices (n, 4, 4) float32, prev_ids (n,) uint32, moved (n,) uint32): moved = 0 when the 16 words of the transform are bit-equal; m = inverse_now *
    transform_then in the row convention (world now -> local -> world then), in double, each dot product summed left to right, rounded to float once.
    (Products of two floats are exact in double, so there is one result whatever fuses what.)"""
    now = np.ascontiguousarray(transform_now, dtype=F).reshape(-1, 4, 4)
    inv = np.ascontiguousarray(inverse_now, dtype=F).reshape(-1, 4, 4).astype(np.float64)
    then = np.ascontiguousarray(transform_then, dtype=F).reshape(-1, 4, 4)
    then64 = then.astype(np.float64)
    m = np.zeros(now.shape, dtype=np.float64)
    for i in range(4):
        for j in range(4):
            s = inv[:, i, 0] * then64[:, 0, j]
            for k in range(1, 4):
                s = s + inv[:, i, k] * then64[:, k, j]
            m[:, i, j] = s
    moved = np.any(now.view(np.uint32).reshape(-1, 16) != then.view(np.uint32).reshape(-1, 16), axis=1)
    return m.astype(F), np.ascontiguousarray(id_then, dtype=np.uint32).reshape(-1), moved.astype(np.uint32)


def where_it_was(normal, position, object_id, object_motion):
    """(N', P', the id then, known): the per-pixel step of the definition"""
    matrices, prev_ids, moved = object_motion
    matrices = np.ascontiguousarray(matrices, dtype=F).reshape(-1, 4, 4)
    prev_ids, moved = np.asarray(prev_ids, dtype=np.uint32).reshape(-1), np.asarray(moved).reshape(-1) != 0
    n = matrices.shape[0]
    assert n >= 1 and prev_ids.shape == moved.shape == (n,)
    ids = np.asarray(object_id, dtype=np.uint32).reshape(normal.shape[1:])
    known = ids < n
    o = np.where(known, ids, 0).astype(np.int64)
    m = matrices[o]                      # (H, W, 4, 4)
    mv = moved[o]
    with np.errstate(all="ignore"):
        p_then, n_then = [], []
        for j in range(3):
            pj = position[0] * m[..., 0, j] + m[..., 3, j]
            pj = position[1] * m[..., 1, j] + pj
            pj = position[2] * m[..., 2, j] + pj
            nj = normal[0] * m[..., 0, j]
            nj = normal[1] * m[..., 1, j] + nj
            nj = normal[2] * m[..., 2, j] + nj
            p_then.append(np.where(mv, pj, position[j]).astype(F))
            n_then.append(np.where(mv, nj, normal[j]).astype(F))
    return np.stack(n_then), np.stack(p_then), prev_ids[o], known


def accumulate_moving(color, color_half, depth, normal, position, albedo=None, object_id=None, history=None, prev_world_to_screen=None,
                      prev_sample_offset=(0.0, 0.0), object_motion=None, **params):
    """temporal_ref.accumulate's arguments and results, with object_motion = (matrices (n, 4, 4), prev_ids (n,), moved (n,)); both id planes are required."""
    assert object_motion is not None and object_id is not None and (history is None or history.get("object_id") is not None)
    color = np.asarray(color, dtype=F)
    h, w = color.shape[:2]
    depth = np.asarray(depth, dtype=F).reshape(h, w)
    normal, position = np.asarray(normal, dtype=F), np.asarray(position, dtype=F)
    ids = np.asarray(object_id, dtype=np.uint32).reshape(h, w)
    n_then, p_then, id_then, known = where_it_was(normal, position, ids, object_motion)
    result, motion, taken, reason = temporal_ref.accumulate(color, color_half, np.where(known, depth, F(np.inf)).astype(F), n_then, p_then, albedo, id_then, history,
                                                           prev_world_to_screen, prev_sample_offset, **params)
    result.update(depth=depth, normal=normal, position=position, object_id=ids)     # the stored history keeps the current N, P and id
    return result, motion, taken, reason


def rigid(rng, max_angle=0.7, max_shift=3.0):
    """a random rigid motion as a row-convention 4 x 4 (float64): rotation about a random axis, then a translation"""
    axis = rng.normal(size=3)
    axis /= np.linalg.norm(axis)
    angle = rng.uniform(0.1, max_angle) * rng.choice([-1.0, 1.0])
    k = np.array([[0.0, -axis[2], axis[1]], [axis[2], 0.0, -axis[0]], [-axis[1], axis[0], 0.0]])
    r = np.eye(3) + np.sin(angle) * k + (1.0 - np.cos(angle)) * (k @ k)
    m = np.eye(4)
    m[:3, :3] = r.T          # row vectors: p' = p @ m
    m[3, :3] = rng.uniform(-max_shift, max_shift, size=3)
    return m


def random_moving_frame(w, h, seed, num_objects=4):
    """temporal_ref.random_temporal_frame with its surface split among 3 .. 5 objects under distinct rigid motions and a permuted id space.  The base frame's
    current guides are taken as where the surface WAS (they lie on the history, with every drop-out the base frame plants); each object's pixels are carried
    to where the object is NOW by the inverse of its motion, so that the table's matrix brings them back -- up to float rounding, which the tap tests'
    margins cover.  Object 0 stands still (moved = 0).  Planted on top: pixels that claim the neighbouring object (their geometry matches the history, the
    id then does not), history pixels of an id no object had, and pixels with an id outside the table.  Returns the base dict plus object_motion and
    `planted`: the masks, for the coverage test."""
    assert 3 <= num_objects <= 5
    base = temporal_ref.random_temporal_frame(w, h, seed)
    rng = np.random.default_rng(seed + 7919)
    cur, prev = base["current"], base["history"]
    n = w * h
    blocks = rng.integers(0, num_objects, size=(max(1, (h + 15) // 16), max(1, (w + 15) // 16)))
    owner = np.kron(blocks, np.ones((16, 16), dtype=np.int64))[:h, :w].copy()
    if n >= 16:
        owner[0, :] = np.arange(w) % num_objects     # (every object shows, whatever the blocks drew)
    perm = rng.permutation(num_objects).astype(np.uint32)
    if np.array_equal(perm, np.arange(num_objects)):
        perm = np.roll(perm, 1)                      # (the id space IS permuted)
    motions = [np.eye(4)] + [rigid(rng) for _ in range(num_objects - 1)]       # current world -> previous world
    matrices = np.stack(motions).astype(F)
    moved = np.array([0] + [1] * (num_objects - 1), dtype=np.uint32)
    pick = lambda share: (rng.random((h, w)) < share) & (n >= 16)   # noqa: E731
    claims_neighbour = cur["object_id"] == 7                           # the base frame's "another object" pixels
    acting = np.where(claims_neighbour, (owner + 1) % num_objects, owner)
    position, normal = cur["position"].astype(np.float64), cur["normal"].astype(np.float64)
    new_position, new_normal = position.copy(), normal.copy()
    for o in range(1, num_objects):
        inverse = np.linalg.inv(motions[o])
        mask = acting == o
        p = np.concatenate([position[:, mask], np.ones((1, int(mask.sum())))]).T @ inverse
        new_position[:, mask] = p[:, :3].T
        new_normal[:, mask] = (normal[:, mask].T @ inverse[:3, :3]).T
    ids = acting.astype(np.uint32)
    outside_table = pick(0.03)
    ids[outside_table] = num_objects + rng.integers(0, 5, size=int(outside_table.sum())).astype(np.uint32)
    ids[~np.isfinite(cur["depth"])] = RT_INVALID_OBJECT                 # a miss, as the OBJECT_ID plane has it
    prev_ids = perm[owner]
    stranger = prev["object_id"] == 9
    prev_ids[stranger] = num_objects + 5
    current = dict(cur, position=new_position.astype(F), normal=new_normal.astype(F), object_id=ids)
    history = dict(prev, object_id=prev_ids.astype(np.uint32))
    planted = dict(claims_neighbour=claims_neighbour & np.isfinite(cur["depth"]) & ~outside_table, outside_table=outside_table & np.isfinite(cur["depth"]), stranger=stranger,
                   moving=(acting != 0) & np.isfinite(cur["depth"]) & ~outside_table, owner=owner)
    return dict(current=current, history=history, prev_world_to_screen=base["prev_world_to_screen"], prev_sample_offset=base["prev_sample_offset"],
                object_motion=(matrices, perm, moved), planted=planted, base=base)
