"""The thin-lens camera ray (include/ptx.h, "thin-lens camera: aperture and focus distance") restated in numpy, from the header's
text.  numpy's binary64 * + - / and sqrt are single IEEE operations, never fused; sin, cos and hypot are the oracle's
(oracle.math_vec, shared pt_math.h mode), so every value here is what the rule says bit for bit.

    lens_rays(cam4, A, F, cxcy, uv) -> (origins (n, 3), directions (n, 3))
    focus_points(cam4, F, cxcy)     -> P = F * q, (n, 3)
"""
import numpy as np

import texture_reference as TR
from envlight_reference import _cos, _sin

PI = TR.PI


def _q(cam4, cxcy):
    llx, lly, vx, vy = (np.float64(c) for c in cam4)
    cxcy = np.asarray(cxcy, dtype=np.float64).reshape(-1, 2)
    return np.stack([llx + (vx * cxcy[:, 0]), lly + (vy * cxcy[:, 1]), np.full(len(cxcy), -1.0)], axis=1)


def focus_points(cam4, F, cxcy):
    return np.float64(F) * _q(cam4, cxcy)


def lens_rays(cam4, A, F, cxcy, uv):
    A = np.float64(A)
    uv = np.asarray(uv, dtype=np.float64).reshape(-1, 2)
    P = focus_points(cam4, F, cxcy)
    r = np.sqrt(uv[:, 0])
    th = (uv[:, 1] * 2.0) * PI
    lx, ly = r * _cos(th), r * _sin(th)
    L = np.stack([A * lx, A * ly, np.zeros(len(uv))], axis=1)
    return L, TR.normalize(P - L)
