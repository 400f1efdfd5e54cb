"""The a-trous filter of include/rtgpu.h (rtgpu_filter_atrous) as a NumPy float32 model: the specification the device is held to bit for bit
(tests/test_gpu_denoise.py); its own properties: tests/test_denoise_model.py.

Vectorised over the pixels, a Python loop over the 25 taps in the stated order (rows outermost).  Every operation is an element-wise float32 one --
no np.sum, no dot -- so each a * b + c is a rounded multiply followed by a rounded add and every sum associates as it is written."""
import numpy as np

F = np.float32
H_WEIGHTS = (F(0.375), F(0.25), F(0.0625))
DEMODULATE = 1


def host_constants(iterations, sigma_color, sigma_normal, sigma_plane):
    """invN, invP, [invC[s]]"""
    sn, sp, sc = F(sigma_normal), F(sigma_plane), F(sigma_color)
    inv_n, inv_p = F(1.0) / (sn * sn), F(1.0) / (sp * sp)
    inv_c = [F(1.0) / (sc * sc)]
    for _ in range(iterations - 1):
        inv_c.append(inv_c[-1] * F(4.0))
    return inv_n, inv_p, inv_c


def atrous(color, depth, normal, position, albedo=None, iterations=5, sigma_color=1.0, sigma_normal=0.25, sigma_plane=0.1, color_scale=1.0, demodulate=True):
    """color (H, W, 3); depth (H, W) or (1, H, W); normal, position, albedo (3, H, W); all float32.  Returns (H, W, 3) float32."""
    color = np.asarray(color, dtype=F)
    h, w = color.shape[:2]
    depth = np.asarray(depth, dtype=F).reshape(h, w)
    normal, position = np.asarray(normal, dtype=F), np.asarray(position, dtype=F)
    assert 1 <= iterations <= 8 and color.shape == (h, w, 3) and normal.shape == (3, h, w) and position.shape == (3, h, w)
    valid = np.isfinite(depth)
    inv_n, inv_p, inv_c = host_constants(iterations, sigma_color, sigma_normal, sigma_plane)
    with np.errstate(all="ignore"):
        # prepare
        c = [color[..., k] * F(color_scale) for k in range(3)]
        d = [np.ones((h, w), dtype=F) for _ in range(3)]
        if demodulate:
            albedo = np.asarray(albedo, dtype=F)
            assert albedo.shape == (3, h, w)
            for k in range(3):
                d[k] = np.where(albedo[k] > F(1e-3), albedo[k], F(1.0)).astype(F)
                c[k] = c[k] / d[k]
        ys, xs = np.mgrid[0:h, 0:w]
        for s in range(iterations):
            step = 1 << s
            acc = [np.zeros((h, w), dtype=F) for _ in range(3)]
            wsum = np.zeros((h, w), dtype=F)
            for j in range(-2, 3):
                for i in range(-2, 3):
                    qx, qy = xs + step * i, ys + step * j
                    inside = (qx >= 0) & (qx < w) & (qy >= 0) & (qy < h)
                    cx, cy = np.where(inside, qx, xs), np.where(inside, qy, ys)   # (a skipped tap reads the pixel itself; its values are dropped)
                    take = inside & valid[cy, cx]
                    nq = [normal[k][cy, cx] for k in range(3)]
                    pq = [position[k][cy, cx] for k in range(3)]
                    cq = [c[k][cy, cx] for k in range(3)]
                    dn = [normal[k] - nq[k] for k in range(3)]
                    dp = [pq[k] - position[k] for k in range(3)]
                    dc = [c[k] - cq[k] for k in range(3)]
                    xn = (dn[0] * dn[0] + dn[1] * dn[1]) + dn[2] * dn[2]
                    t = (normal[0] * dp[0] + normal[1] * dp[1]) + normal[2] * dp[2]
                    xp = t * t
                    xc = (dc[0] * dc[0] + dc[1] * dc[1]) + dc[2] * dc[2]
                    x = (xn * inv_n + xp * inv_p) + xc * inv_c[s]
                    u = np.fmax(F(0.0), F(1.0) - x * F(0.0625))
                    for _ in range(4):
                        u = u * u
                    wt = (H_WEIGHTS[abs(i)] * H_WEIGHTS[abs(j)]) * u
                    for k in range(3):
                        acc[k] = np.where(take, acc[k] + wt * cq[k], acc[k])
                    wsum = np.where(take, wsum + wt, wsum)
            filtered = valid & (wsum != F(0.0))
            c = [np.where(filtered, acc[k] / wsum, c[k]).astype(F) for k in range(3)]
        # finish
        out = np.stack([c[k] * d[k] for k in range(3)], axis=-1)
    assert out.dtype == F
    return out


def random_frame(w, h, seed, invalid=0.1, dark_albedo=0.1):
    """a W x H frame of random inputs: unit normals, `invalid` of the pixels misses (+inf depth, zero guides), `dark_albedo` of the albedo channels below 1e-3"""
    rng = np.random.default_rng(seed)
    color = rng.random((h, w, 3), dtype=F) * F(4.0)
    depth = (rng.random((h, w), dtype=F) * F(10.0) + F(0.5)).astype(F)
    # a few orientations and a few planes, so that taps both pass and stop at the normal and plane terms
    palette = rng.normal(size=(6, 3)).astype(F)
    palette = (palette / np.sqrt((palette * palette).sum(axis=1, keepdims=True))).astype(F)
    pick = rng.integers(0, 6, size=(max(1, (h + 7) // 8), max(1, (w + 7) // 8)))
    pick = np.kron(pick, np.ones((8, 8), dtype=np.int64))[:h, :w]
    normal = np.moveaxis(palette[pick], -1, 0).copy()
    normal = (normal + rng.normal(scale=0.02, size=normal.shape)).astype(F)
    normal = (normal / np.sqrt((normal * normal).sum(axis=0, keepdims=True))).astype(F)
    position = (rng.random((3, h, w), dtype=F) * F(0.2) + np.stack([np.mgrid[0:h, 0:w][1], np.mgrid[0:h, 0:w][0], np.zeros((h, w))]).astype(F) * F(0.01)).astype(F)
    albedo = (rng.random((3, h, w), dtype=F) * F(0.9) + F(0.05)).astype(F)
    albedo[rng.random((3, h, w)) < dark_albedo] = F(5e-4)
    miss = rng.random((h, w)) < invalid
    depth[miss] = np.inf
    normal[:, miss] = 0.0
    position[:, miss] = 0.0
    albedo[:, miss] = 0.0
    return dict(color=color, depth=depth, normal=normal, position=position, albedo=albedo)
