"""History clipping (include/rtgpu.h: "Clipping the history", rtgpu_temporal_accumulate_clip) as a NumPy float32 model: the specification the device is held to bit
for bit (tests/test_gpu_temporal_clip.py); its own properties: tests/test_temporal_clip_model.py.

As tests/temporal_ref.py: vectorised over the pixels, Python loops over the window and over the four taps in the stated order, every operation an element-wise
float32 one -- no np.sum, no dot.  The prepare step's divisor, the start reasons and the per-pixel step of moving objects are the existing models' own
(temporal_ref, temporal_moving_ref); project, taps and blend are restated here because the clip sits between the division by ks and the blend, and
tests/test_temporal_clip_model.py holds the restatement to temporal_moving_ref.accumulate_moving word for word where nothing clips.

Beside the outputs accumulate_clip returns what the device does not: per pixel cnt, whether the pixel clipped, and f (the device's confidence plane)."""
import numpy as np

import temporal_moving_ref
import temporal_ref
from temporal_ref import F, BLENDED, START_NO_HISTORY, START_INVALID, START_OFF_SCREEN, START_NO_TAP, DEFAULTS

CLIP_DEFAULTS = dict(radius=3, gamma=1.0, min_count=9)


def prepare(color, color_half, albedo, color_scale, demodulate):
    """(c, b, d): the prepare step of rtgpu_temporal_accumulate, three (H, W) planes each"""
    h, w = color.shape[:2]
    scale = F(color_scale)
    c = [color[..., k] * scale for k in range(3)]
    b = [color_half[..., k] * (F(2.0) * scale) for k in range(3)]
    d = temporal_ref.divisor(albedo, h, w, demodulate)
    if demodulate:
        c = [c[k] / d[k] for k in range(3)]
        b = [b[k] / d[k] for k in range(3)]
    return [x.astype(F) for x in c], [x.astype(F) for x in b], d


def moments(c, depth, normal, position, object_id, radius, gamma, normal_threshold=DEFAULTS["normal_threshold"], plane_tolerance=DEFAULTS["plane_tolerance"]):
    """`moments` of the definition over prepared colours c (three (H, W) planes) and this frame's guides: (mu, g -- three planes each --, cnt)"""
    h, w = depth.shape
    ys, xs = np.mgrid[0:h, 0:w]
    valid = np.isfinite(depth)
    limit = F(plane_tolerance) * depth
    cnt = np.zeros((h, w), dtype=F)
    s1, s2 = [np.zeros((h, w), dtype=F) for _ in range(3)], [np.zeros((h, w), dtype=F) for _ in range(3)]
    for dy in range(-radius, radius + 1):
        for dx in range(-radius, radius + 1):
            qx, qy = xs + dx, ys + dy
            inside = (qx >= 0) & (qx < w) & (qy >= 0) & (qy < h)
            cx, cy = np.where(inside, qx, xs), np.where(inside, qy, ys)   # (a window pixel outside the frame reads the pixel itself and is dropped)
            nq = [normal[i][cy, cx] for i in range(3)]
            dp = [position[i][cy, cx] - position[i] for i in range(3)]
            cosine = (normal[0] * nq[0] + normal[1] * nq[1]) + normal[2] * nq[2]
            offset = np.abs((normal[0] * dp[0] + normal[1] * dp[1]) + normal[2] * dp[2])
            counts = inside & valid[cy, cx] & (cosine >= F(normal_threshold)) & (offset <= limit)
            if object_id is not None:
                counts = counts & (object_id[cy, cx] == object_id)
            cnt = np.where(counts, cnt + F(1.0), cnt)
            for k in range(3):
                cq = c[k][cy, cx]
                s1[k] = np.where(counts, s1[k] + cq, s1[k])
                s2[k] = np.where(counts, s2[k] + cq * cq, s2[k])
    mu = [s1[k] / cnt for k in range(3)]
    var = [np.fmax(s2[k] / cnt - mu[k] * mu[k], F(0.0)) for k in range(3)]
    g = [F(gamma) * np.sqrt(var[k]) for k in range(3)]
    assert all(x.dtype == F for x in mu + g) and cnt.dtype == F
    return mu, g, cnt


def accumulate_clip(color, color_half, depth, normal, position, albedo=None, object_id=None, history=None, prev_world_to_screen=None, prev_sample_offset=(0.0, 0.0),
                    object_motion=None, clip=None, color_scale=1.0, alpha_min=DEFAULTS["alpha_min"], max_history=DEFAULTS["max_history"],
                    normal_threshold=DEFAULTS["normal_threshold"], plane_tolerance=DEFAULTS["plane_tolerance"], demodulate=True):
    """temporal_moving_ref.accumulate_moving's arguments (object_motion=None: temporal_ref.accumulate's) and clip = dict(radius, gamma, min_count), or None: the
    call without a clip.  Returns (history of this frame, motion (2, H, W), taps taken, start reason, dict(cnt (H, W) float32, clipped (H, W) bool, f (H, W)
    float32))."""
    color, color_half = np.asarray(color, dtype=F), np.asarray(color_half, dtype=F)
    h, w = color.shape[:2]
    depth = np.asarray(depth, dtype=F).reshape(h, w)
    normal, position = np.asarray(normal, dtype=F), np.asarray(position, dtype=F)
    assert color.shape == color_half.shape == (h, w, 3) and normal.shape == (3, h, w) and position.shape == (3, h, w)
    ids = None if object_id is None else np.asarray(object_id, dtype=np.uint32).reshape(h, w)
    ys, xs = np.mgrid[0:h, 0:w]
    with np.errstate(all="ignore"):
        c, b, _ = prepare(color, color_half, albedo, color_scale, demodulate)
        # where the surface point was and which id it had there: the pixel's own, unless objects moved
        n_then, p_then, id_then, known = normal, position, ids, np.ones((h, w), dtype=bool)
        if object_motion is not None:
            assert ids is not None and (history is None or history.get("object_id") is not None)
            n_then, p_then, id_then, known = temporal_moving_ref.where_it_was(normal, position, ids, object_motion)
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
            mu, g, cnt = moments(c, depth, normal, position, ids, radius, gamma, normal_threshold, plane_tolerance)
        if history is not None:
            m = np.asarray(prev_world_to_screen, dtype=F).reshape(4, 4)
            prev_a, prev_b = np.asarray(history["a"], dtype=F), np.asarray(history["b"], dtype=F)
            prev_length = np.asarray(history["length"], dtype=F).reshape(h, w)
            prev_valid = np.isfinite(np.asarray(history["depth"], dtype=F).reshape(h, w))
            prev_normal, prev_position = np.asarray(history["normal"], dtype=F), np.asarray(history["position"], dtype=F)
            prev_id = history.get("object_id")
            assert (prev_id is None) == (ids is None), "the object test needs both id planes"
            # project
            t = []
            for j in range(4):
                tj = p_then[0] * m[0, j] + m[3, j]
                tj = p_then[1] * m[1, j] + tj
                tj = p_then[2] * m[2, j] + tj
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
            limit = F(plane_tolerance) * depth
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
                take = reaches & inside & prev_valid[cy, cx] & (cosine >= F(normal_threshold)) & (offset <= limit)
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
                # clip
                active = blend & (cnt >= F(min_count))
                shift = []
                for i in range(3):
                    lo, hi = mu[i] - g[i], mu[i] + g[i]
                    pulled = np.fmin(np.fmax(ha[i], lo), hi)
                    shift.append(pulled - ha[i])
                    hb[i] = np.where(active, hb[i] + shift[i], hb[i]).astype(F)
                    ha[i] = np.where(active, pulled, ha[i]).astype(F)
                # anti-lag
                e = (np.abs(shift[0]) + np.abs(shift[1])) + np.abs(shift[2])
                wd = (g[0] + g[1]) + g[2]
                clipped = active & (e > F(0.0))
                f = np.where(clipped, wd / (wd + e), F(1.0)).astype(F)
                n = np.fmin((ln / ks) * f + F(1.0), F(max_history))
            else:
                n = np.fmin(ln / ks + F(1.0), F(max_history))
            # blend
            alpha = np.fmax(F(1.0) / n, F(alpha_min))
            for i in range(3):
                out_a[i] = np.where(blend, ha[i] + alpha * (c[i] - ha[i]), c[i]).astype(F)
                out_b[i] = np.where(blend, hb[i] + alpha * (b[i] - hb[i]), b[i]).astype(F)
            length = np.where(blend, n, F(1.0)).astype(F)
            motion = np.stack([np.where(blend, fx - xs.astype(F), F(0.0)), np.where(blend, fy - ys.astype(F), F(0.0))]).astype(F)
            reason = np.where(~valid, START_INVALID, np.where(~on_screen, START_OFF_SCREEN, np.where(~blend, START_NO_TAP, BLENDED)))
        else:
            reason = np.where(valid, START_NO_HISTORY, START_INVALID)
    result = dict(a=np.stack(out_a, axis=-1), b=np.stack(out_b, axis=-1), length=length, depth=depth, normal=normal, position=position, object_id=ids)
    assert result["a"].dtype == result["b"].dtype == length.dtype == motion.dtype == f.dtype == F
    return result, motion, taken, reason, dict(cnt=cnt, clipped=clipped, f=f)
