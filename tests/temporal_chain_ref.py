"""Temporal accumulation over chain guides (include/rtgpu.h: "Temporal accumulation over chain guides", rtgpu_temporal_accumulate_chain) as a NumPy float32 model:
the specification the device is held to bit for bit (tests/test_gpu_temporal_chain.py); its own properties: tests/test_temporal_chain_model.py.  And the rule
of RT_AOV_VIRTUAL_POSITION as a fold over an oracle path recording (tests/test_gpu_virtual_plane.py), on tests/guide_chain_ref.py's fold.

As tests/temporal_clip_ref.py, whose prepare step, moments and start reasons are used as they are: the moments of the chain call are temporal_clip_ref.moments
with chainDistance in depth's place and the chain length folded into the id the window compares (a window pixel counts iff id AND chain length are equal).
project, taps, clip and blend are restated, because the chain's three rules sit inside them; tests/test_temporal_chain_model.py holds the restatement to
temporal_clip_ref.accumulate_clip word for word under k = 0."""
import numpy as np

import temporal_clip_ref
import temporal_moving_ref
from temporal_ref import F, BLENDED, START_NO_HISTORY, START_INVALID, START_OFF_SCREEN, START_NO_TAP, DEFAULTS

START_CHAIN_MOVED = 5   # objects given and chainLength_p > 0: the virtual image of a scene in which something moved is not followed


def chain_moments(c, chain_distance, normal, position, object_id, chain_length, radius, gamma, normal_threshold=DEFAULTS["normal_threshold"],
                  plane_tolerance=DEFAULTS["plane_tolerance"]):
    """`moments` over chain guides: validity and the tolerance's scale from chainDistance, and chainLength_q == chainLength_p beside the id test"""
    key = chain_length.astype(np.uint64) << np.uint64(32)
    if object_id is not None:
        key = key | object_id.astype(np.uint64)
    return temporal_clip_ref.moments(c, chain_distance, normal, position, key, radius, gamma, normal_threshold, plane_tolerance)


def accumulate_chain(color, color_half, depth, normal, position, virtual_position, chain_length, chain_distance, albedo=None, object_id=None, history=None,
                     prev_world_to_screen=None, prev_sample_offset=(0.0, 0.0), object_motion=None, clip=None, color_scale=1.0, alpha_min=DEFAULTS["alpha_min"],
                     max_history=DEFAULTS["max_history"], normal_threshold=DEFAULTS["normal_threshold"], plane_tolerance=DEFAULTS["plane_tolerance"], demodulate=True):
    """temporal_clip_ref.accumulate_clip's arguments and this frame's virtual_position (3, H, W) float32, chain_length (H, W) uint32 and chain_distance (H, W)
    float32; a history carries "chain_length" beside temporal_clip_ref's keys.  Returns what accumulate_clip returns; the history dict carries chain_length."""
    color, color_half = np.asarray(color, dtype=F), np.asarray(color_half, dtype=F)
    h, w = color.shape[:2]
    depth = np.asarray(depth, dtype=F).reshape(h, w)
    normal, position, virtual = np.asarray(normal, dtype=F), np.asarray(position, dtype=F), np.asarray(virtual_position, dtype=F)
    kp = np.asarray(chain_length, dtype=np.uint32).reshape(h, w)
    dist = np.asarray(chain_distance, dtype=F).reshape(h, w)
    assert color.shape == color_half.shape == (h, w, 3) and normal.shape == position.shape == virtual.shape == (3, h, w)
    ids = None if object_id is None else np.asarray(object_id, dtype=np.uint32).reshape(h, w)
    ys, xs = np.mgrid[0:h, 0:w]
    with np.errstate(all="ignore"):
        c, b, _ = temporal_clip_ref.prepare(color, color_half, albedo, color_scale, demodulate)
        # static: the virtual position is projected, the taps are tested against the guide vertex's own pair.  Objects given: a pixel with a chain starts, a
        # pixel without follows the moving rules unchanged -- the moved first-hit pair is projected AND tested
        n_then, p_then, id_then, known, projected = normal, position, ids, np.ones((h, w), dtype=bool), virtual
        if object_motion is not None:
            assert ids is not None and (history is None or history.get("object_id") is not None)
            n_then, p_then, id_then, known = temporal_moving_ref.where_it_was(normal, position, ids, object_motion)
            projected = p_then
            chain_moved = known & np.isfinite(depth) & (kp > 0)
            known = known & (kp == 0)
        valid = np.isfinite(depth) & known
        out_a, out_b = [c[k].copy() for k in range(3)], [b[k].copy() for k in range(3)]
        length = np.ones((h, w), dtype=F)
        motion = np.zeros((2, h, w), dtype=F)
        taken = np.zeros((h, w), dtype=np.int64)
        f = np.ones((h, w), dtype=F)
        clipped = np.zeros((h, w), dtype=bool)
        cnt = np.zeros((h, w), dtype=F)
        if clip is not None:
            radius, gamma, min_count = int(clip["radius"]), clip["gamma"], int(clip["min_count"])
            assert radius in (1, 2, 3) and 1 <= min_count <= 49 and np.isfinite(gamma) and 0.0 <= gamma <= 1e6
            mu, g, cnt = chain_moments(c, dist, normal, position, ids, kp, radius, gamma, normal_threshold, plane_tolerance)
        if history is not None:
            m = np.asarray(prev_world_to_screen, dtype=F).reshape(4, 4)
            prev_a, prev_b = np.asarray(history["a"], dtype=F), np.asarray(history["b"], dtype=F)
            prev_length = np.asarray(history["length"], dtype=F).reshape(h, w)
            prev_valid = np.isfinite(np.asarray(history["depth"], dtype=F).reshape(h, w))
            prev_normal, prev_position = np.asarray(history["normal"], dtype=F), np.asarray(history["position"], dtype=F)
            prev_id = history.get("object_id")
            prev_k = np.asarray(history["chain_length"], dtype=np.uint32).reshape(h, w)
            assert (prev_id is None) == (ids is None), "the object test needs both id planes"
            # project: V_p in P_p's place
            t = []
            for j in range(4):
                tj = projected[0] * m[0, j] + m[3, j]
                tj = projected[1] * m[1, j] + tj
                tj = projected[2] * m[2, j] + tj
                t.append(tj)
            u = (t[0] / t[3]) * F(0.5) + F(0.5)
            v = (t[1] / t[3]) * F(0.5) + F(0.5)
            fx = u * F(w) - F(prev_sample_offset[0])
            fr = v * F(h) - F(prev_sample_offset[1])
            fy = F(h - 1) - fr
            on_screen = (t[2] > F(0.0)) & (fx > F(-1.0)) & (fx < F(w)) & (fy > F(-1.0)) & (fy < F(h))
            reaches = valid & on_screen
            # taps
            sx, sy = np.where(reaches, fx, F(0.0)).astype(F), np.where(reaches, fy, F(0.0)).astype(F)
            flx, fly = np.floor(sx), np.floor(sy)
            tx, ty = sx - flx, sy - fly
            x0, y0 = flx.astype(np.int64), fly.astype(np.int64)
            limit = F(plane_tolerance) * dist   # tolerance: the unfolded path length, not the last segment's
            h_a, h_b = [np.zeros((h, w), dtype=F) for _ in range(3)], [np.zeros((h, w), dtype=F) for _ in range(3)]
            ln, ks = np.zeros((h, w), dtype=F), np.zeros((h, w), dtype=F)
            for tb, ta in ((0, 0), (0, 1), (1, 0), (1, 1)):
                qx, qy = x0 + ta, y0 + tb
                inside = (qx >= 0) & (qx < w) & (qy >= 0) & (qy < h)
                cx, cy = np.where(inside, qx, xs), np.where(inside, qy, ys)
                k = (tx if ta else F(1.0) - tx) * (ty if tb else F(1.0) - ty)
                nq = [prev_normal[i][cy, cx] for i in range(3)]
                dp = [prev_position[i][cy, cx] - p_then[i] for i in range(3)]
                cosine = (n_then[0] * nq[0] + n_then[1] * nq[1]) + n_then[2] * nq[2]
                offset = np.abs((n_then[0] * dp[0] + n_then[1] * dp[1]) + n_then[2] * dp[2])
                take = reaches & inside & prev_valid[cy, cx] & (cosine >= F(normal_threshold)) & (offset <= limit) & (prev_k[cy, cx] == kp)
                if ids is not None:
                    take = take & (np.asarray(prev_id).reshape(h, w)[cy, cx] == id_then)
                for i in range(3):
                    h_a[i] = np.where(take, h_a[i] + k * prev_a[cy, cx, i], h_a[i])
                    h_b[i] = np.where(take, h_b[i] + k * prev_b[cy, cx, i], h_b[i])
                ln = np.where(take, ln + k * prev_length[cy, cx], ln)
                ks = np.where(take, ks + k, ks)
                taken = taken + take
            blend = ks > F(0.0)
            ha, hb = [h_a[i] / ks for i in range(3)], [h_b[i] / ks for i in range(3)]
            if clip is not None:
                active = blend & (cnt >= F(min_count))
                shift = []
                for i in range(3):
                    lo, hi = mu[i] - g[i], mu[i] + g[i]
                    pulled = np.fmin(np.fmax(ha[i], lo), hi)
                    shift.append(pulled - ha[i])
                    hb[i] = np.where(active, hb[i] + shift[i], hb[i]).astype(F)
                    ha[i] = np.where(active, pulled, ha[i]).astype(F)
                e = (np.abs(shift[0]) + np.abs(shift[1])) + np.abs(shift[2])
                wd = (g[0] + g[1]) + g[2]
                clipped = active & (e > F(0.0))
                f = np.where(clipped, wd / (wd + e), F(1.0)).astype(F)
                n = np.fmin((ln / ks) * f + F(1.0), F(max_history))
            else:
                n = np.fmin(ln / ks + F(1.0), F(max_history))
            alpha = np.fmax(F(1.0) / n, F(alpha_min))
            for i in range(3):
                out_a[i] = np.where(blend, ha[i] + alpha * (c[i] - ha[i]), c[i]).astype(F)
                out_b[i] = np.where(blend, hb[i] + alpha * (b[i] - hb[i]), b[i]).astype(F)
            length = np.where(blend, n, F(1.0)).astype(F)
            motion = np.stack([np.where(blend, fx - xs.astype(F), F(0.0)), np.where(blend, fy - ys.astype(F), F(0.0))]).astype(F)
            reason = np.where(~valid, START_INVALID, np.where(~on_screen, START_OFF_SCREEN, np.where(~blend, START_NO_TAP, BLENDED)))
            if object_motion is not None:
                reason = np.where(chain_moved, START_CHAIN_MOVED, reason)
        else:
            reason = np.where(valid, START_NO_HISTORY, START_INVALID)
    result = dict(a=np.stack(out_a, axis=-1), b=np.stack(out_b, axis=-1), length=length, depth=depth, normal=normal, position=position, object_id=ids, chain_length=kp)
    assert result["a"].dtype == result["b"].dtype == length.dtype == motion.dtype == f.dtype == F
    return result, motion, taken, reason, dict(cnt=cnt, clipped=clipped, f=f)


# ---- RT_AOV_VIRTUAL_POSITION over an oracle path recording -----------------------------------------------------------------------------------------
def virtual_position(vertices, desc, max_chain):
    """include/rtgpu.h, "The virtual position", over an (n, 28) recording: the (3,) float32 plane words.  o and w: words 0..2 and 3..5 of vertex 0; k and D:
    guide_chain_ref.fold.  k == 0: the guide vertex's position (words 11..13), zero where the reference leaves them unwritten, as the POSITION plane is."""
    import guide_chain_ref
    import path_records_ref
    k, distance, _ = guide_chain_ref.fold(vertices, desc, max_chain)
    if np.isinf(distance):
        return np.zeros(3, dtype=F)
    if k == 0:
        stale = path_records_ref.stale_mask(vertices, desc)[0]
        return np.where(stale[11:14], F(0.0), vertices[0, 11:14]).astype(F)
    with np.errstate(all="ignore"):
        o, w = vertices[0, 0:3].astype(F), vertices[0, 3:6].astype(F)
        return (o + (w * F(distance)).astype(F)).astype(F)


def virtual_frame(frame, desc, max_chain):
    """virtual_position of every pixel of a guide_chain_ref.oracle_frame: (P, 3) float32"""
    return np.stack([virtual_position(vertices, desc, max_chain) for vertices in frame])
