"""Sphere light sampling (include/ptx.h, "cone-sampling emissive spheres in PTX_LIGHTING_SAMPLED") restated in numpy, from the header's
text.  numpy's binary64 * + - / and sqrt are single IEEE operations, never fused; the rule's explicit fused multiply-adds (V3.dot,
V3.cross) are `fma` below -- an error-free product, a round-to-odd sum and one final rounding (Boldo and Melquiond), exact rational
arithmetic wherever an operand is outside the range that construction is proved for; sin, cos and hypot are the oracle's
(oracle.math_vec, shared pt_math.h mode).  So every value here is what the rule says bit for bit.

    table(tri, spheres)              -> Table: the joined table of light triangles ((n, 9) vertices) and emissive spheres ((n, 4))
    sample(tab, points, uv)          -> (world-space unit directions (n, 3), the entry drawn (n,))
    pd(tab, points, dirs)            -> densities per solid angle (n,)
"""
from collections import namedtuple
from fractions import Fraction

import numpy as np

import texture_reference as TR

PI = TR.PI
FN_HYPOT, FN_SIN, FN_COS = 0, 1, 2  # ptx_math_eval's numbering
MAX_FINITE = 1.7976931348623157e308
Table = namedtuple("Table", "tri sph cum total")  # tri (nt, 14), sph (ns, 8), cum (nt + ns,), W_total


def _mv(fn, a, b=None):
    from oracle import oracle as O
    a = np.ascontiguousarray(a, dtype=np.float64)
    return O.math_vec(fn, a, None if b is None else np.ascontiguousarray(b, dtype=np.float64))


# ------------------------------------------------------------------------------------------------ fused multiply-add
def _two_sum(a, b):
    s = a + b
    bb = s - a
    return s, (a - (s - bb)) + (b - bb)


def _split(a):
    c = 134217729.0 * a
    hi = c - (c - a)
    return hi, a - hi


def _two_prod(a, b):
    p = a * b
    ah, al = _split(a)
    bh, bl = _split(b)
    return p, ((ah * bh - p) + ah * bl + al * bh) + al * bl


def _fma_exact(a, b, c):
    return float(Fraction(a) * Fraction(b) + Fraction(c))


def fma(a, b, c):
    """round(a * b + c), one rounding, elementwise"""
    a, b, c = np.broadcast_arrays(np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64), np.asarray(c, dtype=np.float64))
    a, b, c = a.ravel().copy(), b.ravel().copy(), c.ravel().copy()
    with np.errstate(all="ignore"):
        plain = a * b + c  # right whenever the product is exact (zeros, signed zeros), and for anything not finite
        p, e = _two_prod(a, b)
        th, tl = _two_sum(c, p)
        v, verr = _two_sum(tl, e)
        even = (v.view(np.int64) & 1) == 0
        v = np.where((verr != 0.0) & even, np.nextafter(v, np.where(verr > 0.0, np.inf, -np.inf)), v)  # round to odd
        out = th + v
        finite = np.isfinite(a) & np.isfinite(b) & np.isfinite(c) & np.isfinite(plain)
        lo, hi = 2.0 ** -450, 2.0 ** 450
        safe = ((np.abs(a) > lo) & (np.abs(a) < hi) & (np.abs(b) > lo) & (np.abs(b) < hi)
                & ((c == 0.0) | ((np.abs(c) > 2.0 ** -900) & (np.abs(c) < 2.0 ** 900))))
        out = np.where(finite & safe & (e != 0.0), out, plain)
        slow = np.nonzero(finite & ~safe & (a != 0.0) & (b != 0.0))[0]
    for i in slow:
        out[i] = _fma_exact(float(a[i]), float(b[i]), float(c[i]))
    return out


# ------------------------------------------------------------------------------------------------ V3, Quaternion, Shader_space
def dot(v, w):
    return fma(v[0], w[0], fma(v[1], w[1], v[2] * w[2]))


def _h(w, x, y, z):
    return fma(w, x, -(y * z))


def cross(p, q):
    return (_h(p[1], q[2], p[2], q[1]), _h(p[2], q[0], p[0], q[2]), _h(p[0], q[1], p[1], q[0]))


def sub(a, b):
    return (a[0] - b[0], a[1] - b[1], a[2] - b[2])


def add(a, b):
    return (a[0] + b[0], a[1] + b[1], a[2] + b[2])


def scale(v, s):
    return (s * v[0], s * v[1], s * v[2])


def normalize(v):
    with np.errstate(all="ignore"):
        s = 1.0 / _mv(FN_HYPOT, v[0], _mv(FN_HYPOT, v[1], v[2]))
        return scale(v, s)


def quat_mul(a, b):
    r = (a[0] * b[0]) - dot(a[1], b[1])
    v = add(add(cross(a[1], b[1]), scale(b[1], a[0])), scale(a[1], b[0]))
    return (r, v)


def quat_conj(q):
    return (q[0], (-q[1][0], -q[1][1], -q[1][2]))


def quat_transform(t, v):
    zero = np.zeros_like(v[0])
    return quat_mul(quat_mul(t, (zero, v)), quat_conj(t))[1]


def shader_rotation(n):
    """Shader_space.create's rotation with Quaternion.normalize (shader_space.ml:11-23, quaternion.ml:11-15)"""
    eps = 1e-9
    x, y, z = n
    with np.errstate(all="ignore"):
        r = 1.0 + z
        vx, vy, vz = y, -x, np.zeros_like(x)
        s = 1.0 / _mv(FN_HYPOT, _mv(FN_HYPOT, r, vx), _mv(FN_HYPOT, vy, vz))
        up, down = z > 1.0 - eps, z < eps - 1.0
        one, zero = np.ones_like(x), np.zeros_like(x)
        qr = np.where(up, one, np.where(down, zero, r * s))
        qx = np.where(up | down, zero, s * vx)
        qy = np.where(up, zero, np.where(down, one, s * vy))
        qz = np.where(up | down, zero, s * vz)
    return (qr, (qx, qy, qz))


def rotate_inv(n, v):
    return quat_transform(quat_conj(shader_rotation(n)), v)


# ------------------------------------------------------------------------------------------------ the table
def table(tri, spheres):
    """tri: (nt, 9) the light triangles' vertices a, b, c in list order; spheres: (ns, 4) {x, y, z, r} in list order"""
    tri = np.asarray(tri, dtype=np.float64).reshape(-1, 9)
    sph = np.asarray(spheres, dtype=np.float64).reshape(-1, 4)
    T = np.zeros((len(tri), 14))
    cum = 0.0
    for k in range(len(tri)):
        a, b, c = ([np.array([t]) for t in tri[k, 3 * i:3 * i + 3]] for i in range(3))
        cr = cross(sub(b, a), sub(c, a))
        n = normalize(cr)
        area = 0.5 * np.sqrt(dot(cr, cr))[0]
        cum = cum + area
        T[k, :9] = tri[k]
        T[k, 9:12] = [n[0][0], n[1][0], n[2][0]]
        T[k, 12], T[k, 13] = area, cum
    S = np.zeros((len(sph), 8))
    for k in range(len(sph)):
        r2 = sph[k, 3] * sph[k, 3]
        W = (2.0 * PI) * r2
        cum = cum + W
        S[k, :4] = sph[k]
        S[k, 4], S[k, 5], S[k, 6] = r2, W, cum
    return Table(T, S, np.concatenate([T[:, 13], S[:, 6]]), float(cum))


def _q(r2, d2):
    s2 = r2 / d2
    return s2 / (1.0 + np.sqrt(1.0 - s2))


def sample(tab, points, uv):
    p = np.asarray(points, dtype=np.float64).reshape(-1, 3)
    uv = np.asarray(uv, dtype=np.float64).reshape(-1, 2)
    nt, n = len(tab.tri), len(tab.cum)
    P = (p[:, 0], p[:, 1], p[:, 2])
    v = uv[:, 1]
    with np.errstate(all="ignore"):
        x = (2.0 * uv[:, 0]) * tab.total
        above = x[:, None] < tab.cum[None, :]
        k = np.where(above.any(axis=1), above.argmax(axis=1), n - 1)
        before = np.where(k > 0, tab.cum[np.maximum(k - 1, 0)], 0.0)
        weight = np.concatenate([tab.tri[:, 12], tab.sph[:, 5]])[k]
        q = (x - before) / weight
        u2 = np.where(np.isnan(q), np.nan, np.minimum(q, 1.0))
        out = np.zeros((len(p), 3))
        if nt:
            L = tab.tri[np.minimum(k, nt - 1)]
            s = np.sqrt(u2)
            b1, b2 = 1.0 - s, v * s
            b0 = 1.0 - b1 - b2
            pt = [(b0 * L[:, i] + b1 * L[:, 3 + i]) + b2 * L[:, 6 + i] for i in range(3)]
            d = normalize(sub(pt, P))
            out = np.stack(d, axis=1)
        if n > nt:
            S = tab.sph[np.clip(k - nt, 0, n - nt - 1)]
            r2 = S[:, 4]
            f = sub((S[:, 0], S[:, 1], S[:, 2]), P)
            d2 = dot(f, f)
            phi = (v * 2.0) * PI
            sn, cs = _mv(FN_SIN, phi), _mv(FN_COS, phi)
            z = 1.0 - 2.0 * u2
            m = 1.0 - z * z
            sq = np.sqrt(np.where(m > 0.0, m, 0.0))
            inside = (sq * cs, sq * sn, z)
            t = u2 * _q(r2, d2)
            ct, st = 1.0 - t, np.sqrt(t * (2.0 - t))
            outside = rotate_inv(normalize(f), (st * cs, st * sn, ct))
            w = np.stack([np.where(d2 <= r2, inside[i], outside[i]) for i in range(3)], axis=1)
            out = np.where((k >= nt)[:, None], w, out)
    return out, k.astype(np.int32)


def _triangle_t(a, b, c, o, d):
    """Triangle.intersect on [0, max_float]: (hit, t)"""
    e1, e2 = sub(b, a), sub(c, a)
    pvec = cross(d, e2)
    det = dot(e1, pvec)
    det_inv = 1.0 / det
    tvec = sub(o, a)
    u = det_inv * dot(tvec, pvec)
    qvec = cross(tvec, e1)
    v = det_inv * dot(d, qvec)
    t = det_inv * dot(e2, qvec)
    hit = ~(np.abs(det) < 1e-6) & (0.0 <= u) & (u <= 1.0) & (0.0 <= v) & (u + v <= 1.0) & (0.0 <= t) & (t <= MAX_FINITE)
    return hit, t


def pd(tab, points, dirs):
    p = np.asarray(points, dtype=np.float64).reshape(-1, 3)
    w = np.asarray(dirs, dtype=np.float64).reshape(-1, 3)
    P, Wd = (p[:, 0], p[:, 1], p[:, 2]), (w[:, 0], w[:, 1], w[:, 2])
    acc = np.zeros(len(p))
    ones = np.ones(len(p))
    with np.errstate(all="ignore"):
        for L in tab.tri:
            a, b, c, n = ([L[3 * i + j] * ones for j in range(3)] for i in range(4))
            hit, t = _triangle_t(a, b, c, P, Wd)
            term = (t * t) / (tab.total * np.abs(dot(n, Wd)))
            acc = np.where(hit, acc + term, acc)
        for S in tab.sph:
            r2, share = S[4], S[5] / tab.total
            f = sub((S[0] * ones, S[1] * ones, S[2] * ones), P)
            d2 = dot(f, f)
            bp = dot(f, Wd)
            g = sub(f, scale(Wd, bp))
            cone = (bp > 0.0) & (r2 - dot(g, g) >= 0.0)
            acc = np.where(d2 <= r2, acc + share / (4.0 * PI), np.where(cone, acc + share / ((2.0 * PI) * _q(r2, d2)), acc))
    return acc
