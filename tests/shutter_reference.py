"""The camera shutter's ray (include/ptx.h, "camera shutter: motion blur between two poses") restated in numpy, from the header's text.
numpy's binary64 * + - / and sqrt are single IEEE operations, never fused; sin, cos and hypot are the oracle's (oracle.math_vec,
shared pt_math.h mode), so every value here is what the rule says bit for bit.

    shutter_rays(cam4, origin, rotation, T, k, A, cxcy, t, lens=None, uv=None, latlong=False) -> (origins (n, 3), directions (n, 3))
    lens = (radius, F) with uv (n, 2) the lens pairs, or None; latlong: the panorama's vector for the frustum's (cam4 is not read)
    dimension(max_bounces, lens) -> d;  the time is dimension d - 1 and the lens pair d - 3 and d - 2
    rotation_matrix(k, a) -> Rot(k, a) in closed form (NOT the rule's arithmetic: what the rule is compared against)
"""
import numpy as np

import texture_reference as TR
from camera_pose_reference import rotate
from envlight_reference import _cos, _sin

PI = TR.PI


def dimension(max_bounces, lens):
    return 2 + 2 * max_bounces + (2 if lens else 0) + 1


def turn(k, sn, cs, oc, w):
    """S(w).i = ((w.i * cs) + (c.i * sn)) + (k.i * (kw * oc))"""
    kx, ky, kz = (np.float64(c) for c in k)
    kw = (kx * w[:, 0] + ky * w[:, 1]) + kz * w[:, 2]
    c = np.stack([(ky * w[:, 2]) - (kz * w[:, 1]), (kz * w[:, 0]) - (kx * w[:, 2]), (kx * w[:, 1]) - (ky * w[:, 0])], axis=1)
    ko = kw * oc
    return np.stack([((w[:, i] * cs) + (c[:, i] * sn)) + (kk * ko) for i, kk in enumerate((kx, ky, kz))], axis=1)


def shutter_rays(cam4, origin, rotation, T, k, A, cxcy, t, lens=None, uv=None, latlong=False):
    o = np.asarray(origin, dtype=np.float64).reshape(3)
    T = np.asarray(T, dtype=np.float64).reshape(3)
    k = np.asarray(k, dtype=np.float64).reshape(3)
    cxcy = np.asarray(cxcy, dtype=np.float64).reshape(-1, 2)
    n = len(cxcy)
    t = np.broadcast_to(np.asarray(t, dtype=np.float64), (n,))
    a = t * np.float64(A)
    sn, cs = _sin(a), _cos(a)
    oc = 1.0 - cs
    ot = np.stack([o[i] + (t * T[i]) for i in range(3)], axis=1)
    if latlong:
        u = cxcy[:, 0]
        v = 1.0 - cxcy[:, 1]
        al = u * (2.0 * PI) - PI
        th = v * PI
        sa, ca, st, ct = _sin(al), _cos(al), _sin(th), _cos(th)
        e = np.stack([st * ca, -ct, -(st * sa)], axis=1)
        return ot, TR.normalize(turn(k, sn, cs, oc, rotate(rotation, e)))
    llx, lly, vx, vy = (np.float64(c) for c in cam4)
    q = np.stack([llx + (vx * cxcy[:, 0]), lly + (vy * cxcy[:, 1]), np.full(n, -1.0)], axis=1)
    if lens is None:
        return ot, TR.normalize(turn(k, sn, cs, oc, rotate(rotation, q)))
    radius, F = np.float64(lens[0]), np.float64(lens[1])
    uv = np.asarray(uv, dtype=np.float64).reshape(-1, 2)
    P = F * q
    r = np.sqrt(uv[:, 0])
    th = (uv[:, 1] * 2.0) * PI
    lx, ly = r * _cos(th), r * _sin(th)
    L = np.stack([radius * lx, radius * ly, np.zeros(n)], axis=1)
    e = P - L
    return ot + turn(k, sn, cs, oc, rotate(rotation, L)), TR.normalize(turn(k, sn, cs, oc, rotate(rotation, e)))


def rotation_matrix(k, a):
    """Rot(k, a) = cos a I + sin a [k]x + (1 - cos a) k k^T, entry by entry in closed form (libm's sin and cos)"""
    x, y, z = (float(c) for c in k)
    c, s = np.cos(a), np.sin(a)
    v = 1.0 - c
    return np.array([[c + x * x * v, x * y * v - z * s, x * z * v + y * s],
                     [y * x * v + z * s, c + y * y * v, y * z * v - x * s],
                     [z * x * v - y * s, z * y * v + x * s, c + z * z * v]])
