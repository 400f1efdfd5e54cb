"""The variance-guided a-trous filter of include/rtgpu.h (rtgpu_filter_atrous_var) as a NumPy float32 model: the specification the device is held to bit
for bit (tests/test_gpu_denoise_var.py); its own properties: tests/test_denoise_var_model.py.

As tests/denoise_ref.py: vectorised over the pixels, Python loops over the 9 taps of the local-variance window and the 25 taps of a level in the stated
order (rows outermost), every operation an element-wise float32 one -- no np.sum, no dot."""
import numpy as np

from denoise_ref import DEMODULATE, F, H_WEIGHTS, random_frame   # noqa: F401

G_WEIGHTS = (F(0.5), F(0.25))
DEFAULTS = dict(sigma_lum=4.0, variance_floor=1e-10)


def lum(c):
    return ((c[0] + F(2.0) * c[1]) + c[2]) * F(0.25)


def host_constants(sigma_lum, sigma_normal, sigma_plane):
    """invN, invP, sL2"""
    sn, sp, sl = F(sigma_normal), F(sigma_plane), F(sigma_lum)
    return F(1.0) / (sn * sn), F(1.0) / (sp * sp), sl * sl


def atrous_var(color, color_half, depth, normal, position, albedo=None, iterations=5, sigma_lum=DEFAULTS["sigma_lum"], sigma_normal=0.25, sigma_plane=0.1,
               variance_floor=DEFAULTS["variance_floor"], color_scale=1.0, demodulate=True):
    """color, color_half (H, W, 3); depth (H, W) or (1, H, W); normal, position, albedo (3, H, W); all float32.  Returns the (H, W, 3) image and the (H, W)
    variance, both float32."""
    color, color_half = np.asarray(color, dtype=F), np.asarray(color_half, dtype=F)
    h, w = color.shape[:2]
    depth = np.asarray(depth, dtype=F).reshape(h, w)
    normal, position = np.asarray(normal, dtype=F), np.asarray(position, dtype=F)
    assert 1 <= iterations <= 8 and color.shape == color_half.shape == (h, w, 3) and normal.shape == (3, h, w) and position.shape == (3, h, w)
    valid = np.isfinite(depth)
    inv_n, inv_p, sl2 = host_constants(sigma_lum, sigma_normal, sigma_plane)
    floor = F(variance_floor)
    with np.errstate(all="ignore"):
        # prepare
        scale = F(color_scale)
        c = [color[..., k] * scale for k in range(3)]
        b = [color_half[..., k] * (F(2.0) * scale) for k in range(3)]
        d = [np.ones((h, w), dtype=F) for _ in range(3)]
        if demodulate:
            albedo = np.asarray(albedo, dtype=F)
            assert albedo.shape == (3, h, w)
            for k in range(3):
                d[k] = np.where(albedo[k] > F(1e-3), albedo[k], F(1.0)).astype(F)
                c[k] = c[k] / d[k]
                b[k] = b[k] / d[k]
        e = lum(c) - lum(b)
        v = np.where(valid, e * e, F(0.0)).astype(F)
        ys, xs = np.mgrid[0:h, 0:w]
        for s in range(iterations):
            step = 1 << s
            # the local variance: 3 x 3, not dilated
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
            g = gsum / gw   # (0 / 0 at an invalid pixel, which does not use it)
            denom = g * sl2 + floor
            lum_p = lum(c)
            acc = [np.zeros((h, w), dtype=F) for _ in range(3)]
            vacc, wsum = np.zeros((h, w), dtype=F), np.zeros((h, w), dtype=F)
            for j in range(-2, 3):
                for i in range(-2, 3):
                    qx, qy = xs + step * i, ys + step * j
                    inside = (qx >= 0) & (qx < w) & (qy >= 0) & (qy < h)
                    cx, cy = np.where(inside, qx, xs), np.where(inside, qy, ys)   # (a skipped tap reads the pixel itself; its values are dropped)
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
        # finish
        out = np.stack([c[k] * d[k] for k in range(3)], axis=-1)
    assert out.dtype == F and v.dtype == F
    return out, v


def random_frame_var(w, h, seed, invalid=0.1, dark_albedo=0.1, agree=0.1, outliers=3):
    """random_frame(w, h, seed) and a `color_half`: about half of the colour plus noise; at `agree` of the pixels exactly half of it (the two halves agree:
    v = 0); at up to `outliers` pixels the colour is 1e4 times larger, with the half-sample sum left as it was (a firefly in the other half)"""
    f = random_frame(w, h, seed, invalid=invalid, dark_albedo=dark_albedo)
    rng = np.random.default_rng(seed + 77)
    half = (f["color"] * F(0.5)).astype(F)
    noisy = (half + rng.normal(scale=0.15, size=half.shape).astype(F) * half).astype(F)
    same = rng.random((h, w)) < agree
    f["color_half"] = np.where(same[..., None], half, noisy).astype(F)
    for _ in range(min(outliers, (w * h) // 16)):
        y, x = int(rng.integers(0, h)), int(rng.integers(0, w))
        f["color"][y, x] = f["color"][y, x] * F(1e4)
    return f
