"""The a-trous rule of ptx_denoise_device (include/ptx.h) restated in numpy, operation for operation.

Every sum over taps is an explicit loop in row-major tap order (j outer, i inner) that starts at 0 -- never np.sum, whose pairwise
order is not the rule's -- and every expression keeps the header's grouping, so the result is the library's bit for bit (numpy's
binary64 +, -, *, / round as the GPU's do; nothing here contracts a product into an add).  A tap outside the image is skipped: for a
pixel it simply adds nothing, which the shifted-slice form below does by leaving that pixel's accumulators alone."""
import numpy as np

DEMODULATE = 1
DEFAULTS = dict(levels=5, normal_power_log2=5, feature_passes=8, flags=DEMODULATE, sigma_luminance=4.0, sigma_depth=0.05,
                sigma_albedo=0.2)
H5 = (0.0625, 0.25, 0.375, 0.25, 0.0625)
B3 = (0.25, 0.5, 0.25)


def _windows(H, W, dx, dy):
    """(destination slices, source slices) of the pixels p whose tap q = p + (dx, dy) lies in the image, or None"""
    x0, x1 = max(0, -dx), min(W, W - dx)
    y0, y1 = max(0, -dy), min(H, H - dy)
    if x0 >= x1 or y0 >= y1:
        return None
    return (slice(y0, y1), slice(x0, x1)), (slice(y0 + dy, y1 + dy), slice(x0 + dx, x1 + dx))


def prepare(raw, err, feat, k, kf, flags):
    """raw, err: (H, W, 3); feat: (H, W, 8) sums; k: int or (H, W) int array.  Returns a, n, z, h, D, c, V."""
    kd = np.asarray(k, dtype=np.float64)
    kd = kd[..., None] if kd.ndim == 2 else kd
    kfd = float(kf)
    m = raw / kd
    var = err * err
    a = feat[..., 0:3] / kfd
    n = feat[..., 3:6] / kfd
    z = feat[..., 6] / kfd
    h = feat[..., 7]
    D = np.where(a > 2.0 ** -7, a, 1.0) if (flags & DEMODULATE) else np.ones_like(a)
    c = m / D
    V = (var[..., 0] / (D[..., 0] * D[..., 0]) + var[..., 1] / (D[..., 1] * D[..., 1])) + var[..., 2] / (D[..., 2] * D[..., 2])
    return a, n, z, h, D, c, V


def level(c, V, a, n, z, h, step, m, sl, sz, sa):
    H, W = V.shape
    lam = (c[..., 0] + c[..., 1]) + c[..., 2]
    vbar = np.zeros((H, W))
    for j in (-1, 0, 1):
        for i in (-1, 0, 1):
            win = _windows(H, W, i, j)
            if win is None:
                continue
            d, s = win
            vbar[d] = vbar[d] + (B3[j + 1] * B3[i + 1]) * V[s]
    den = (sl * sl) * vbar + 1e-12
    sw = np.zeros((H, W))
    sc = np.zeros((H, W, 3))
    sv = np.zeros((H, W))
    sa2 = sa * sa
    with np.errstate(all="ignore"):
        for j in range(-2, 3):
            for i in range(-2, 3):
                win = _windows(H, W, step * i, step * j)
                if win is None:
                    continue
                d, s = win
                dot = (n[d][..., 0] * n[s][..., 0] + n[d][..., 1] * n[s][..., 1]) + n[d][..., 2] * n[s][..., 2]
                wn = np.where(dot > 0.0, dot, 0.0)
                for _ in range(m):
                    wn = wn * wn
                wn = np.where((h[d] == 0.0) & (h[s] == 0.0), 1.0, wn)
                r = (z[d] - z[s]) / (sz * (np.abs(z[d]) + np.abs(z[s])) + 1e-300)
                wz = 1.0 / (1.0 + r * r)
                e = a[d] - a[s]
                wa = 1.0 / (1.0 + ((e[..., 0] * e[..., 0] + e[..., 1] * e[..., 1]) + e[..., 2] * e[..., 2]) / sa2)
                t = lam[d] - lam[s]
                wl = 1.0 / (1.0 + (t * t) / den[d])
                w = (H5[j + 2] * H5[i + 2]) * (((wn * wz) * wa) * wl)
                sw[d] = sw[d] + w
                sc[d] = sc[d] + w[..., None] * c[s]
                sv[d] = sv[d] + (w * w) * V[s]
    return sc / sw[..., None], sv / (sw * sw)


def denoise(raw, err, feat, k, kf, levels=5, normal_power_log2=5, flags=DEMODULATE, sigma_luminance=4.0, sigma_depth=0.05,
            sigma_albedo=0.2, feature_passes=None, return_variance=False):
    """Denoised SUMS (H, W, 3) on the scale of `raw` = mean * k(p).  levels = 0 returns a copy of raw."""
    raw = np.ascontiguousarray(raw, dtype=np.float64)
    if levels == 0:
        return (raw.copy(), None) if return_variance else raw.copy()
    a, n, z, h, D, c, V = prepare(raw, np.asarray(err, dtype=np.float64), np.asarray(feat, dtype=np.float64), k, kf, flags)
    for l in range(levels):
        c, V = level(c, V, a, n, z, h, 1 << l, normal_power_log2, sigma_luminance, sigma_depth, sigma_albedo)
    kd = np.asarray(k, dtype=np.float64)
    kd = kd[..., None] if kd.ndim == 2 else kd
    out = (c * D) * kd
    return (out, V) if return_variance else out


def standard_error(s1, s2, k):
    """ptx_pixel_error_device's se from the sums and the squares' sums after k passes (k >= 2), per channel"""
    kd = np.asarray(k, dtype=np.float64)
    kd = kd[..., None] if kd.ndim == 2 else kd
    v = s2 - s1 * s1 / kd
    return np.sqrt(np.where(v > 0.0, v, 0.0) / (kd * (kd - 1.0)))
