"""The posed camera's ray (include/ptx.h, "camera pose: a movable camera, no rebuild") restated in numpy, from the header's text.
numpy's binary64 * + - / and sqrt are single IEEE operations, never fused; sin, cos and hypot are the oracle's (oracle.math_vec,
shared pt_math.h mode), so every value here is what the rule says bit for bit.

    pose_rays(cam4, origin, rotation, cxcy, lens=None, uv=None) -> (origins (n, 3), directions (n, 3))
    lens = (A, F) with uv (n, 2) the lens pairs, or None for no lens
"""
import numpy as np

import texture_reference as TR
from envlight_reference import _cos, _sin

PI = TR.PI
IDENTITY = np.eye(3)


def rotate(R, a):
    """Rv(a) = ((r00 a.x + r01 a.y) + r02 a.z, ...)"""
    R = np.asarray(R, dtype=np.float64).reshape(3, 3)
    return np.stack([(R[i, 0] * a[:, 0] + R[i, 1] * a[:, 1]) + R[i, 2] * a[:, 2] for i in range(3)], axis=1)


def pose_rays(cam4, origin, rotation, cxcy, lens=None, uv=None):
    llx, lly, vx, vy = (np.float64(c) for c in cam4)
    o = np.asarray(origin, dtype=np.float64).reshape(3)
    cxcy = np.asarray(cxcy, dtype=np.float64).reshape(-1, 2)
    n = len(cxcy)
    q = np.stack([llx + (vx * cxcy[:, 0]), lly + (vy * cxcy[:, 1]), np.full(n, -1.0)], axis=1)
    if lens is None:
        return np.tile(o, (n, 1)), TR.normalize(rotate(rotation, q))
    A, F = np.float64(lens[0]), np.float64(lens[1])
    uv = np.asarray(uv, dtype=np.float64).reshape(-1, 2)
    P = F * q
    r = np.sqrt(uv[:, 0])
    th = (uv[:, 1] * 2.0) * PI
    lx, ly = r * _cos(th), r * _sin(th)
    L = np.stack([A * lx, A * ly, np.zeros(n)], axis=1)
    e = P - L
    return o[None, :] + rotate(rotation, L), TR.normalize(rotate(rotation, e))
