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
