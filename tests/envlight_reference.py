"""Environment sampling (include/ptx.h, "importance-sampling the environment in PTX_LIGHTING_SAMPLED") restated in numpy, from the
header's text.  numpy's binary64 * + / are single IEEE operations, never fused; running sums are explicit left-to-right loops (np.cumsum
over an axis adds in that order too, but the loop is what the rule says); sin, cos, atan2, acos and hypot are the oracle's
(oracle.math_vec, shared pt_math.h mode), so every value here is what the rule says bit for bit.

    density(img)                     -> Density(w, c, m, T, last_row, last_col)
    sample(den, R, ab)               -> (unit directions (n, 3), texels (n, 2) as (ix, iy))
    pd(den, R, dirs)                 -> (densities per solid angle (n,), the texels looked up (n, 2))
"""
from collections import namedtuple

import numpy as np

import texture_reference as TR

PI = TR.PI
FN_SIN, FN_COS = 1, 2  # ptx_math_eval's numbering
Density = namedtuple("Density", "w c m T last_row last_col")


def _sin(x):
    from oracle import oracle as O
    return O.math_vec(FN_SIN, np.ascontiguousarray(x, dtype=np.float64))


def _cos(x):
    from oracle import oracle as O
    return O.math_vec(FN_COS, np.ascontiguousarray(x, dtype=np.float64))


def density(img):
    img = np.asarray(img, dtype=np.float64)
    H, W = img.shape[:2]
    lum = (img[:, :, 0] + img[:, :, 1]) + img[:, :, 2]
    lum = np.where(lum > 0.0, lum, 0.0)
    s = _sin(PI * ((np.arange(H, dtype=np.float64) + 0.5) / np.float64(H)))
    w = lum * s[:, None]
    c = np.zeros((H, W))
    run = np.zeros(H)
    for ix in range(W):
        run = run + w[:, ix]
        c[:, ix] = run
    r = c[:, W - 1]
    m = np.zeros(H)
    total = 0.0
    for iy in range(H):
        total = total + r[iy]
        m[iy] = total
    rows = np.nonzero(r > 0.0)[0]
    last_row = int(rows[-1]) if len(rows) else 0
    last_col = np.array([int(np.nonzero(w[iy] > 0.0)[0][-1]) if (w[iy] > 0.0).any() else 0 for iy in range(H)])
    return Density(w, c, m, float(total), last_row, last_col)


def _first_above(table, x, fallback):
    """per element: the first index k with x < table[k] (table: (n, K) rows or (K,)), `fallback` where there is none"""
    above = x[:, None] < (table if table.ndim == 2 else table[None, :])
    return np.where(above.any(axis=1), above.argmax(axis=1), fallback)


def sample(den, R, ab):
    ab = np.asarray(ab, dtype=np.float64).reshape(-1, 2)
    R = np.eye(3).reshape(-1) if R is None else np.asarray(R, dtype=np.float64).reshape(-1)
    H, W = den.w.shape
    a, b = ab[:, 0], ab[:, 1]
    with np.errstate(invalid="ignore", divide="ignore"):
        x = a * den.T
        iy = _first_above(den.m, x, den.last_row)
        before = np.where(iy > 0, den.m[np.maximum(iy - 1, 0)], 0.0)
        r = den.c[iy, W - 1]
        fy = np.minimum((x - before) / r, 1.0)
        y = b * r
        ix = _first_above(den.c[iy], y, den.last_col[iy])
        before = np.where(ix > 0, den.c[iy, np.maximum(ix - 1, 0)], 0.0)
        fx = np.minimum((y - before) / den.w[iy, ix], 1.0)
    u = (ix.astype(np.float64) + fx) / np.float64(W)
    v = (iy.astype(np.float64) + fy) / np.float64(H)
    al, th = u * (2.0 * PI) - PI, v * PI
    sa, ca, st, ct = _sin(al), _cos(al), _sin(th), _cos(th)
    m = [st * ca, -ct, -(st * sa)]
    d = np.stack([(R[k] * m[0] + R[3 + k] * m[1]) + R[6 + k] * m[2] for k in range(3)], axis=1)
    return TR.normalize(d), np.stack([ix, iy], axis=1).astype(np.int32)


def pd(den, R, dirs):
    H, W = den.w.shape
    u, v = TR.environment_uv(dirs, R)
    with np.errstate(invalid="ignore", divide="ignore"):
        ix = np.minimum(np.maximum(np.trunc(TR._scale(u, W)).astype(np.int64), 0), W - 1)
        iy = np.minimum(np.maximum(np.trunc(TR._scale(v, H)).astype(np.int64), 0), H - 1)
        st = _sin(v * PI)
        val = ((den.w[iy, ix] / den.T) * (np.float64(W) * np.float64(H))) / ((2.0 * (PI * PI)) * st)
        out = np.where(st > 0.0, val, 0.0)
    return out, np.stack([ix, iy], axis=1).astype(np.int32)
