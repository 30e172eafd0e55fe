"""The image rule and the environment of include/ptx.h ("image textures and a lat-long environment map") restated in numpy, from the
header's text.  numpy's binary64 * and + are single IEEE operations, never fused; the environment's atan2, acos and hypot are the
oracle's (oracle.math_vec, shared pt_math.h mode), so every value here is what the rule says bit for bit.

    image_eval(img, flags, u, v)          img: (H, W, 3) texels, row 0 = v 0
    environment_uv(dirs, R) / environment_eval(img, flags, R, dirs)
    checker_image(W, H, even, odd)        the image that equals Texture.checker (W + 1) (H + 1) for even W, H
    checker_parity(W, H, u, v)            Texture.checker's own rule: 0 = even, 1 = odd
"""
import numpy as np

BILINEAR, REPEAT_U, REPEAT_V = 1, 2, 4
MAX_SIZE = 16384
PI = 3.14159265358979323846
FN_HYPOT, FN_ACOS, FN_ATAN2 = 0, 3, 4  # ptx_math_eval's numbering


def _scale(u, n):
    """p = u * n; a product that is NaN or not below 2^62 in magnitude is replaced by 0"""
    with np.errstate(invalid="ignore", over="ignore"):
        p = np.asarray(u, dtype=np.float64) * np.float64(n)
        return np.where(np.abs(p) < 2.0 ** 62, p, 0.0)


def _wrap(i, n, repeat):
    i = np.asarray(i, dtype=np.int64)
    if repeat:
        return ((np.fmod(i, n)) + n) % n  # C's %: the sign of the dividend; the second % makes it non-negative
    return np.minimum(np.maximum(i, 0), n - 1)


def _lerp(a, b, t):
    t = t[:, None]
    return a * (1.0 - t) + b * t


def image_eval(img, flags, u, v):
    img = np.asarray(img, dtype=np.float64)
    H, W = img.shape[:2]
    u, v = np.atleast_1d(np.asarray(u, dtype=np.float64)), np.atleast_1d(np.asarray(v, dtype=np.float64))
    rep_u, rep_v = bool(flags & REPEAT_U), bool(flags & REPEAT_V)
    p, q = _scale(u, W), _scale(v, H)
    if not flags & BILINEAR:
        ix = _wrap(np.trunc(p).astype(np.int64), W, rep_u)
        iy = _wrap(np.trunc(q).astype(np.int64), H, rep_v)
        return img[iy, ix]
    x, y = p - 0.5, q - 0.5
    x0, y0 = np.floor(x), np.floor(y)
    fx, fy = x - x0, y - y0
    ix0, ix1 = _wrap(x0.astype(np.int64), W, rep_u), _wrap(x0.astype(np.int64) + 1, W, rep_u)
    iy0, iy1 = _wrap(y0.astype(np.int64), H, rep_v), _wrap(y0.astype(np.int64) + 1, H, rep_v)
    top = _lerp(img[iy0, ix0], img[iy0, ix1], fx)
    bot = _lerp(img[iy1, ix0], img[iy1, ix1], fx)
    return _lerp(top, bot, fy)


def normalize(d):
    """V3.normalize: scale v (1 / hypot x (hypot y z))"""
    from oracle import oracle as O
    d = np.asarray(d, dtype=np.float64).reshape(-1, 3)
    with np.errstate(divide="ignore", invalid="ignore"):
        s = 1.0 / O.math_vec(FN_HYPOT, d[:, 0].copy(), O.math_vec(FN_HYPOT, d[:, 1].copy(), d[:, 2].copy()))
        return s[:, None] * d


def environment_uv(dirs, R=None):
    from oracle import oracle as O
    R = np.eye(3).reshape(-1) if R is None else np.asarray(R, dtype=np.float64).reshape(-1)
    e = normalize(dirs)
    m = [(R[3 * k] * e[:, 0] + R[3 * k + 1] * e[:, 1]) + R[3 * k + 2] * e[:, 2] for k in range(3)]
    u = (PI + O.math_vec(FN_ATAN2, -m[2], m[0])) * (1.0 / (2.0 * PI))
    v = O.math_vec(FN_ACOS, -np.minimum(np.maximum(m[1], -1.0), 1.0)) * (1.0 / PI)
    return u, v


def environment_eval(img, flags, R, dirs):
    """of the flags only BILINEAR matters: an environment repeats in u and clamps in v"""
    u, v = environment_uv(dirs, R)
    return image_eval(img, (flags & BILINEAR) | REPEAT_U, u, v)


def checker_image(W, H, even, odd):
    iy, ix = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    same = ((ix & 1) == (iy & 1))[:, :, None]
    return np.where(same, np.asarray(even, dtype=np.float64), np.asarray(odd, dtype=np.float64))


def checker_parity(W, H, u, v):
    """Texture.checker ~width:(W + 1) ~height:(H + 1) (texture.ml:16-31): Float.to_int (u * W) land 1 against the same of v"""
    px = np.trunc(np.asarray(u, dtype=np.float64) * np.float64(W)).astype(np.int64) & 1
    py = np.trunc(np.asarray(v, dtype=np.float64) * np.float64(H)).astype(np.int64) & 1
    return (px != py).astype(np.int64)


def edge_coordinates(W, H, rng, n_random):
    """(u, v) pairs: random in [-3, 3], and every pair of the edge values -- texel edges and centres, 0, 1, 1 - 2^-53, -0.0, just
    outside, negative, up to +-3"""
    def axis(n):
        k = np.arange(-n, 2 * n + 1)
        grid = np.unique(np.concatenate([k / n, (k + 0.5) / n, np.nextafter(k / n, 10.0), np.nextafter(k / n, -10.0)]))
        special = np.array([0.0, -0.0, 1.0, 1.0 - 2.0 ** -53, -2.0 ** -53, 1.0 + 2.0 ** -52, 3.0, -3.0, 2.5, -2.5])
        return np.concatenate([grid, special])  # (np.unique would fold -0.0 into 0.0)
    au, av = axis(W), axis(H)
    gu, gv = np.meshgrid(au, av, indexing="ij")
    ru, rv = rng.uniform(-3.0, 3.0, n_random), rng.uniform(-3.0, 3.0, n_random)
    return np.concatenate([gu.ravel(), ru]), np.concatenate([gv.ravel(), rv])


def limit_coordinates(n, rng):
    """coordinates for an axis of n texels, n up to MAX_SIZE, where edge_coordinates' grid would be too large: random values in
    [-3, 3]; the first and last texel edges with their nextafter neighbours; k 2^32 / n with its neighbours, k = 1..8, both signs
    (where the 64-bit index leaves 32 bits); +-2^61 / n and (2^62 - 2^10) / n (the last products that still count); random values
    with |u n| in [2^31, 2^33].  A few thousand values."""
    def around(x):
        x = np.asarray(x, dtype=np.float64)
        return np.concatenate([x, np.nextafter(x, np.inf), np.nextafter(x, -np.inf)])
    edges = around(np.array([0.0, 1.0, n - 1.0, float(n), -1.0, -(n - 1.0), -float(n), 0.5, n - 0.5]) / n)
    k = np.arange(1.0, 9.0)
    big = around(np.concatenate([k, -k]) * 2.0 ** 32 / n)
    last = around(np.array([2.0 ** 61, -2.0 ** 61, 2.0 ** 62 - 2.0 ** 10, -(2.0 ** 62 - 2.0 ** 10)]) / n)
    below = rng.uniform(2.0 ** 31, 2.0 ** 32, 600) * rng.choice([-1.0, 1.0], 600) / n
    above = rng.uniform(2.0 ** 32, 2.0 ** 33, 600) * rng.choice([-1.0, 1.0], 600) / n
    return np.concatenate([rng.uniform(-3.0, 3.0, 1500), edges, np.array([-0.0]), big, last, below, above])


LIMIT_SIZES = [(16384, 1), (1, 16384), (16383, 2), (12289, 1), (4099, 3)]  # (W, H)


def limit_case(W, H):
    """(img, u, v) of the rule tests at the size limit: the axis coordinates of both axes, paired in a seeded shuffle, and the
    conditions that make the case one -- from the reference's own p = u * n, on the axis that is long, at least 200 coordinates with
    2^32 <= |p| < 2^62 and at least 200 with 2^31 <= |p| < 2^32"""
    rng = np.random.default_rng(W * 7 + H)
    img = rng.uniform(0.0, 4.0, (H, W, 3))
    u, v = limit_coordinates(W, rng), limit_coordinates(H, rng)
    assert len(u) == len(v) and len(u) < 6000
    v = v[rng.permutation(len(v))]
    for c, n in ((u, W), (v, H)):
        p = np.abs(c * np.float64(n))
        assert ((p >= 2.0 ** 32) & (p < 2.0 ** 62)).sum() >= 200 and ((p >= 2.0 ** 31) & (p < 2.0 ** 32)).sum() >= 200, (W, H, n)
    return img, u, v
