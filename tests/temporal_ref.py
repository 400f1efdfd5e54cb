"""Temporal accumulation of include/rtgpu.h (rtgpu_temporal_accumulate) as a NumPy float32 model: the specification the device is held to bit for bit
(tests/test_gpu_temporal.py); its own properties: tests/test_temporal_model.py.

As tests/denoise_var_ref.py: vectorised over the pixels, a Python loop over the four taps in the stated order, every operation an element-wise float32
one -- no np.sum, no dot.  Beside the outputs it returns what the device does not: per pixel the number of taps taken and why a pixel started.

atrous_var_prepared is denoise_var_ref.atrous_var under RT_DENOISE_INPUT_PREPARED: the prepare step skipped, the rest the same text."""
import numpy as np

from denoise_ref import F, H_WEIGHTS, random_frame
from denoise_var_ref import G_WEIGHTS, DEFAULTS as VAR_DEFAULTS, host_constants, lum

DEFAULTS = dict(alpha_min=0.1, max_history=64.0, normal_threshold=0.9, plane_tolerance=0.01)
# why a pixel started (0: it did not): the order the definition tests in
BLENDED, START_NO_HISTORY, START_INVALID, START_OFF_SCREEN, START_NO_TAP = 0, 1, 2, 3, 4


def divisor(albedo, h, w, demodulate):
    """d_k of the definition"""
    if not demodulate:
        return [np.ones((h, w), dtype=F) for _ in range(3)]
    albedo = np.asarray(albedo, dtype=F)
    assert albedo.shape == (3, h, w)
    return [np.where(albedo[k] > F(1e-3), albedo[k], F(1.0)).astype(F) for k in range(3)]


def accumulate(color, color_half, depth, normal, position, albedo=None, object_id=None, history=None, prev_world_to_screen=None, prev_sample_offset=(0.0, 0.0),
               color_scale=1.0, alpha_min=DEFAULTS["alpha_min"], max_history=DEFAULTS["max_history"], normal_threshold=DEFAULTS["normal_threshold"],
               plane_tolerance=DEFAULTS["plane_tolerance"], demodulate=True):
    """color, color_half (H, W, 3); depth (H, W) or (1, H, W); normal, position, albedo (3, H, W), float32; object_id (H, W) uint32 or None.  history: None, or
    a dict a, b (H, W, 3), length (H, W), depth, normal, position and object_id (or None) of the previous frame -- what this function returns.  Returns
    (history of this frame, motion (2, H, W), taps taken (H, W) int, start reason (H, W) int)."""
    color, color_half = np.asarray(color, dtype=F), np.asarray(color_half, dtype=F)
    h, w = color.shape[:2]
    depth = np.asarray(depth, dtype=F).reshape(h, w)
    normal, position = np.asarray(normal, dtype=F), np.asarray(position, dtype=F)
    assert color.shape == color_half.shape == (h, w, 3) and normal.shape == (3, h, w) and position.shape == (3, h, w)
    valid = np.isfinite(depth)
    ys, xs = np.mgrid[0:h, 0:w]
    with np.errstate(all="ignore"):
        # prepare
        scale = F(color_scale)
        c = [color[..., k] * scale for k in range(3)]
        b = [color_half[..., k] * (F(2.0) * scale) for k in range(3)]
        if demodulate:
            d = divisor(albedo, h, w, True)
            c = [c[k] / d[k] for k in range(3)]
            b = [b[k] / d[k] for k in range(3)]
        out_a, out_b = [c[k].astype(F) for k in range(3)], [b[k].astype(F) for k in range(3)]
        length = np.ones((h, w), dtype=F)
        motion = np.zeros((2, h, w), dtype=F)
        taken = np.zeros((h, w), dtype=np.int64)
        reason = np.full((h, w), START_NO_HISTORY, dtype=np.int64)
        if history is not None:
            m = np.asarray(prev_world_to_screen, dtype=F).reshape(4, 4)
            prev_a, prev_b = np.asarray(history["a"], dtype=F), np.asarray(history["b"], dtype=F)
            prev_length = np.asarray(history["length"], dtype=F).reshape(h, w)
            prev_valid = np.isfinite(np.asarray(history["depth"], dtype=F).reshape(h, w))
            prev_normal, prev_position = np.asarray(history["normal"], dtype=F), np.asarray(history["position"], dtype=F)
            assert prev_a.shape == prev_b.shape == (h, w, 3) and prev_normal.shape == prev_position.shape == (3, h, w)
            prev_id = history.get("object_id")
            assert (prev_id is None) == (object_id is None), "the object test needs both id planes"
            # project
            t = []
            for j in range(4):
                tj = position[0] * m[0, j] + m[3, j]
                tj = position[1] * m[1, j] + tj
                tj = position[2] * m[2, j] + tj
                t.append(tj)
            u = (t[0] / t[3]) * F(0.5) + F(0.5)
            v = (t[1] / t[3]) * F(0.5) + F(0.5)
            fx = u * F(w) - F(prev_sample_offset[0])
            fr = v * F(h) - F(prev_sample_offset[1])
            fy = F(h - 1) - fr
            on_screen = (t[2] > F(0.0)) & (fx > F(-1.0)) & (fx < F(w)) & (fy > F(-1.0)) & (fy < F(h))   # (False for a NaN)
            reaches = valid & on_screen
            # taps (a pixel that does not reach the previous frame takes none: its coordinates are not converted)
            sx, sy = np.where(reaches, fx, F(0.0)).astype(F), np.where(reaches, fy, F(0.0)).astype(F)
            flx, fly = np.floor(sx), np.floor(sy)
            tx, ty = sx - flx, sy - fly
            x0, y0 = flx.astype(np.int64), fly.astype(np.int64)
            limit = F(plane_tolerance) * depth
            h_a, h_b = [np.zeros((h, w), dtype=F) for _ in range(3)], [np.zeros((h, w), dtype=F) for _ in range(3)]
            ln, ks = np.zeros((h, w), dtype=F), np.zeros((h, w), dtype=F)
            for tb, ta in ((0, 0), (0, 1), (1, 0), (1, 1)):   # (a, b) = (0,0), (1,0), (0,1), (1,1)
                qx, qy = x0 + ta, y0 + tb
                inside = (qx >= 0) & (qx < w) & (qy >= 0) & (qy < h)
                cx, cy = np.where(inside, qx, xs), np.where(inside, qy, ys)   # (a skipped tap reads the pixel itself; its values are dropped)
                k = (tx if ta else F(1.0) - tx) * (ty if tb else F(1.0) - ty)
                nq = [prev_normal[i][cy, cx] for i in range(3)]
                dp = [prev_position[i][cy, cx] - position[i] for i in range(3)]
                cosine = (normal[0] * nq[0] + normal[1] * nq[1]) + normal[2] * nq[2]
                offset = np.abs((normal[0] * dp[0] + normal[1] * dp[1]) + normal[2] * dp[2])
                take = reaches & inside & prev_valid[cy, cx] & (cosine >= F(normal_threshold)) & (offset <= limit)
                if object_id is not None:
                    take = take & (np.asarray(prev_id).reshape(h, w)[cy, cx] == np.asarray(object_id).reshape(h, w))
                for i in range(3):
                    h_a[i] = np.where(take, h_a[i] + k * prev_a[cy, cx, i], h_a[i])
                    h_b[i] = np.where(take, h_b[i] + k * prev_b[cy, cx, i], h_b[i])
                ln = np.where(take, ln + k * prev_length[cy, cx], ln)
                ks = np.where(take, ks + k, ks)
                taken = taken + take
            blend = ks > F(0.0)
            # blend
            n = np.fmin(ln / ks + F(1.0), F(max_history))
            alpha = np.fmax(F(1.0) / n, F(alpha_min))
            for i in range(3):
                ha, hb = h_a[i] / ks, h_b[i] / ks
                out_a[i] = np.where(blend, ha + alpha * (c[i] - ha), c[i]).astype(F)
                out_b[i] = np.where(blend, hb + alpha * (b[i] - hb), b[i]).astype(F)
            length = np.where(blend, n, F(1.0)).astype(F)
            motion = np.stack([np.where(blend, fx - xs.astype(F), F(0.0)), np.where(blend, fy - ys.astype(F), F(0.0))]).astype(F)
            reason = np.where(~valid, START_INVALID, np.where(~on_screen, START_OFF_SCREEN, np.where(~blend, START_NO_TAP, BLENDED)))
        else:
            reason = np.where(valid, START_NO_HISTORY, START_INVALID)
    result = dict(a=np.stack(out_a, axis=-1), b=np.stack(out_b, axis=-1), length=length, depth=depth, normal=normal, position=position,
                  object_id=None if object_id is None else np.asarray(object_id).reshape(h, w))
    assert result["a"].dtype == result["b"].dtype == length.dtype == motion.dtype == F
    return result, motion, taken, reason


def remodulate(a, albedo, demodulate=True):
    """rtgpu_denoise_temporal without a filter: outA_k * d_k"""
    a = np.asarray(a, dtype=F)
    h, w = a.shape[:2]
    d = divisor(albedo, h, w, demodulate)
    return np.stack([a[..., k] * d[k] for k in range(3)], axis=-1)


def atrous_var_prepared(c_in, b_in, depth, normal, position, albedo=None, iterations=5, sigma_lum=VAR_DEFAULTS["sigma_lum"], sigma_normal=0.25, sigma_plane=0.1,
                        variance_floor=VAR_DEFAULTS["variance_floor"], demodulate=True):
    """rtgpu_filter_atrous_var with RT_DENOISE_INPUT_PREPARED: c_in, b_in (H, W, 3) are c and b themselves -- no colorScale, no doubling, no division; the
    levels as in denoise_var_ref.atrous_var; the finish multiplies by d under demodulate.  Returns the (H, W, 3) image and the (H, W) variance."""
    c_in, b_in = np.asarray(c_in, dtype=F), np.asarray(b_in, dtype=F)
    h, w = c_in.shape[:2]
    depth = np.asarray(depth, dtype=F).reshape(h, w)
    normal, position = np.asarray(normal, dtype=F), np.asarray(position, dtype=F)
    assert 1 <= iterations <= 8 and c_in.shape == b_in.shape == (h, w, 3) and normal.shape == (3, h, w) and position.shape == (3, h, w)
    valid = np.isfinite(depth)
    inv_n, inv_p, sl2 = host_constants(sigma_lum, sigma_normal, sigma_plane)
    floor = F(variance_floor)
    with np.errstate(all="ignore"):
        c = [c_in[..., k].copy() for k in range(3)]
        b = [b_in[..., k] for k in range(3)]
        d = divisor(albedo, h, w, demodulate)
        e = lum(c) - lum(b)
        v = np.where(valid, e * e, F(0.0)).astype(F)
        ys, xs = np.mgrid[0:h, 0:w]
        for s in range(iterations):
            step = 1 << s
            gsum, gw = np.zeros((h, w), dtype=F), np.zeros((h, w), dtype=F)
            for j in range(-1, 2):
                for i in range(-1, 2):
                    qx, qy = xs + i, ys + j
                    inside = (qx >= 0) & (qx < w) & (qy >= 0) & (qy < h)
                    cx, cy = np.where(inside, qx, xs), np.where(inside, qy, ys)
                    take = inside & valid[cy, cx]
                    k = G_WEIGHTS[abs(i)] * G_WEIGHTS[abs(j)]
                    gsum = np.where(take, gsum + k * v[cy, cx], gsum)
                    gw = np.where(take, gw + k, gw)
            denom = (gsum / gw) * sl2 + floor
            lum_p = lum(c)
            acc = [np.zeros((h, w), dtype=F) for _ in range(3)]
            vacc, wsum = np.zeros((h, w), dtype=F), np.zeros((h, w), dtype=F)
            for j in range(-2, 3):
                for i in range(-2, 3):
                    qx, qy = xs + step * i, ys + step * j
                    inside = (qx >= 0) & (qx < w) & (qy >= 0) & (qy < h)
                    cx, cy = np.where(inside, qx, xs), np.where(inside, qy, ys)
                    take = inside & valid[cy, cx]
                    nq = [normal[k][cy, cx] for k in range(3)]
                    pq = [position[k][cy, cx] for k in range(3)]
                    cq = [c[k][cy, cx] for k in range(3)]
                    vq = v[cy, cx]
                    dn = [normal[k] - nq[k] for k in range(3)]
                    dp = [pq[k] - position[k] for k in range(3)]
                    xn = (dn[0] * dn[0] + dn[1] * dn[1]) + dn[2] * dn[2]
                    t = (normal[0] * dp[0] + normal[1] * dp[1]) + normal[2] * dp[2]
                    xp = t * t
                    dl = lum_p - lum(cq)
                    xc = (dl * dl) / denom
                    x = (xn * inv_n + xp * inv_p) + xc
                    u = np.fmax(F(0.0), F(1.0) - x * F(0.0625))
                    for _ in range(4):
                        u = u * u
                    wt = (H_WEIGHTS[abs(i)] * H_WEIGHTS[abs(j)]) * u
                    for k in range(3):
                        acc[k] = np.where(take, acc[k] + wt * cq[k], acc[k])
                    vacc = np.where(take, vacc + (wt * wt) * vq, vacc)
                    wsum = np.where(take, wsum + wt, wsum)
            filtered = valid & (wsum != F(0.0))
            c = [np.where(filtered, acc[k] / wsum, c[k]).astype(F) for k in range(3)]
            v = np.where(filtered, vacc / (wsum * wsum), v).astype(F)
        out = np.stack([c[k] * d[k] for k in range(3)], axis=-1)
    assert out.dtype == F and v.dtype == F
    return out, v


def affine_world_to_screen(w, h, shift):
    """a prevWorldToScreen with t_3 = 1 and t_2 = P.z that sends position (x, y, z) of a W x H frame to fx = x + shift[0], fy = y + shift[1] (up to rounding):
    u = fx / W means t_0 = 2 * fx / W - 1; film rows run bottom-up: fr = H - 1 - fy, t_1 = 2 * fr / H - 1"""
    m = np.zeros((4, 4), dtype=F)
    m[0, 0], m[3, 0] = 2.0 / w, 2.0 * shift[0] / w - 1.0
    m[1, 1], m[3, 1] = -2.0 / h, 2.0 * (h - 1 - shift[1]) / h - 1.0
    m[2, 2] = 1.0
    m[3, 3] = 1.0
    return m


def random_temporal_frame(w, h, seed, shift=(0.3, -0.6)):
    """A current frame, a history and the affine prevWorldToScreen between them, for the device-against-model tests: smooth guides in patches (so that most
    pixels take all four taps), and every way a tap or a pixel drops out at a rate the coverage test of tests/test_temporal_model.py holds it to.
      position  (x + noise, y + noise, z) with z > 0: the matrix of affine_world_to_screen reprojects pixel x to x + shift + noise
      invalid   misses in both frames (independently); behind: z < 0 at some pixels; outside: a few positions thrown far off the frame; one NaN position
      no tap    blocks of pixels whose normal, plane or object id disagrees with the whole history around them
      partial   single history pixels invalidated or given another id"""
    rng = np.random.default_rng(seed)
    f = random_frame(w, h, seed, invalid=0.0)
    ys, xs = np.mgrid[0:h, 0:w]
    n = w * h
    # one plane facing +z: normals (0, 0, 1) with a little noise; positions on it
    normal = np.zeros((3, h, w), dtype=F)
    normal[2] = 1.0
    normal = (normal + rng.normal(scale=0.002, size=normal.shape)).astype(F)
    normal = (normal / np.sqrt((normal * normal).sum(axis=0, keepdims=True))).astype(F)
    z = (F(2.0) + rng.random((h, w), dtype=F) * F(0.001)).astype(F)
    position = np.stack([xs + rng.normal(scale=0.3, size=(h, w)), ys + rng.normal(scale=0.3, size=(h, w)), z]).astype(F)
    depth = (rng.random((h, w), dtype=F) * F(4.0) + F(1.0)).astype(F)
    ids = rng.integers(0, 3, size=(max(1, (h + 15) // 16), max(1, (w + 15) // 16))).astype(np.uint32)
    ids = np.kron(ids, np.ones((16, 16), dtype=np.uint32))[:h, :w].copy()
    prev = dict(depth=(rng.random((h, w), dtype=F) * F(4.0) + F(1.0)).astype(F), normal=normal.copy(),
                position=np.stack([xs, ys, np.full((h, w), 2.0)]).astype(F), object_id=ids.copy(),
                a=(rng.random((h, w, 3), dtype=F) * F(3.0)).astype(F), b=(rng.random((h, w, 3), dtype=F) * F(3.0)).astype(F),
                length=np.floor(rng.random((h, w)) * 80.0 + 1.0).astype(F))
    cur_ids = ids.copy()
    pick = lambda share: (rng.random((h, w)) < share) & (n >= 16)   # noqa: E731  (a frame of a few pixels keeps them all)
    # whole pixels that find no tap: the normal turned away, the plane offset, another object
    turned = pick(0.04)
    normal[:, turned] = np.array([1.0, 0.0, 0.0], dtype=F)[:, None]
    lifted = pick(0.04) & ~turned
    position[2, lifted] += F(1.0)
    cur_ids[pick(0.04)] = 7
    # behind the camera, off the frame, not a number
    behind = pick(0.05)
    position[2, behind] = F(-1.0)
    outside = pick(0.05) & ~behind
    position[0, outside] += F(4.0 * w + 10.0)
    # single history pixels that drop out of their neighbours' taps
    gone = pick(0.06)
    prev["depth"][gone] = np.inf
    prev["object_id"][pick(0.04)] = 9
    # misses of this frame
    miss = pick(0.08)
    depth[miss] = np.inf
    normal[:, miss] = 0.0
    position[:, miss] = 0.0
    f["albedo"][:, miss] = 0.0
    if n >= 16:   # (a hit whose position is not a number)
        depth[h // 2, w // 2], normal[:, h // 2, w // 2], position[:, h // 2, w // 2] = F(2.0), np.array([0.0, 0.0, 1.0], dtype=F), np.array([np.nan, 1.0, 2.0], dtype=F)
    half = (f["color"] * F(0.5)).astype(F)
    color_half = (half + rng.normal(scale=0.15, size=half.shape).astype(F) * half).astype(F)
    cur = dict(color=f["color"], color_half=color_half, depth=depth, normal=normal, position=position, albedo=f["albedo"], object_id=cur_ids)
    return dict(current=cur, history=prev, prev_world_to_screen=affine_world_to_screen(w, h, (shift[0] + 0.25, shift[1] + 0.125)), prev_sample_offset=(0.25, -0.125))
