"""The lat-long projection's ray (include/ptx.h, "camera projection: a lat-long panorama") restated in numpy, from the header's text.
numpy's binary64 * + - / are single IEEE operations, never fused; sin, cos and hypot are the oracle's (oracle.math_vec, shared
pt_math.h mode), so every value here is what the rule says bit for bit.

    latlong_rays(origin, rotation, cxcy)        -> (origins (n, 3), directions (n, 3))
    film_coordinates(width, height, spp, dim, xs, ys, passes) -> (cxcy (n, 2), jitter (n, 2)) under the sampler's own jitter
    product_latlong_rays(origin, rotation, cxcy) -> the same from csrc/pt_projection.h compiled for the host
"""
import ctypes as C
import os

import numpy as np

import lens_support as LS
import texture_reference as TR
from camera_pose_reference import rotate
from envlight_reference import _cos, _sin

PI = TR.PI
ROOT = LS.ROOT
_PRODUCT = None


def latlong_rays(origin, rotation, cxcy):
    o = np.asarray(origin, dtype=np.float64).reshape(3)
    cxcy = np.asarray(cxcy, dtype=np.float64).reshape(-1, 2)
    u = cxcy[:, 0]
    v = 1.0 - cxcy[:, 1]
    al = u * (2.0 * PI) - PI
    th = v * PI
    sa, ca, st, ct = _sin(al), _cos(al), _sin(th), _cos(th)
    e = np.stack([st * ca, -ct, -(st * sa)], axis=1)
    return np.tile(o, (len(cxcy), 1)), TR.normalize(rotate(rotation, e))


def film_coordinates(width, height, spp, dim, xs, ys, passes):
    """sample_pixel's film coordinates (integrator.ml:96-109): cx = (x + dx) * (1 / W), cy = 1 - ((y + dy) * (1 / H)), (dx, dy) the
    sampler's dimensions 0 and 1 at offset y W + x + pass spp"""
    from oracle import oracle as O
    xs, ys, passes = (np.asarray(a, dtype=np.int64) for a in (xs, ys, passes))
    off = ys * width + xs + passes * spp
    dx = O.lds_get_vec(dim, off, np.zeros(len(off), dtype=np.int64))
    dy = O.lds_get_vec(dim, off, np.ones(len(off), dtype=np.int64))
    widthf, heightf = 1.0 / np.float64(width), 1.0 / np.float64(height)
    cx = (xs.astype(np.float64) + dx) * widthf
    cy = 1.0 - ((ys.astype(np.float64) + dy) * heightf)
    return np.stack([cx, cy], axis=1), np.stack([dx, dy], axis=1)


_PRODUCT_SRC = """
#include "pt_projection.h"
extern "C" void product_latlong_rays(const double* o, const double* R, long long n, const double* cxcy, double* out) {
  PtCameraPose cp;
  for (int i = 0; i < 3; ++i) cp.o[i] = o[i];
  for (int i = 0; i < 9; ++i) cp.r[i] = R[i];
  cp.llx = cp.lly = cp.vx = cp.vy = 0.0 / 0.0; /* the view is not read */
  for (long long i = 0; i < n; ++i) {
    V3 ro, rd;
    pt_latlong_ray(cp, cxcy[2 * i], cxcy[2 * i + 1], &ro, &rd);
    out[6 * i] = ro.x; out[6 * i + 1] = ro.y; out[6 * i + 2] = ro.z; out[6 * i + 3] = rd.x; out[6 * i + 4] = rd.y; out[6 * i + 5] = rd.z;
  }
}
"""


def product():
    """csrc/pt_projection.h -- the function the kernels call -- compiled for the host with the library's floating-point flags"""
    global _PRODUCT
    if _PRODUCT is not None:
        return _PRODUCT
    csrc = os.path.join(ROOT, "path_tracer_ocaml_amd", "csrc")
    deps = [os.path.join(csrc, f) for f in ("pt_projection.h", "pt_camera_pose.h", "pt_vec.h", "pt_math.h")] + [os.path.abspath(__file__)]
    out_dir = os.path.join(ROOT, "build")
    os.makedirs(out_dir, exist_ok=True)
    src = os.path.join(out_dir, "projection_product.cpp")

    def cmd(tmp):
        with open(src, "w") as f:
            f.write(_PRODUCT_SRC)
        return [os.environ.get("CXX", "g++"), "-std=c++17", "-O2", "-fPIC", "-ffp-contract=off", "-fno-fast-math", "-march=x86-64-v3",
                "-I", csrc, "-shared", "-o", tmp, src]
    dp = C.POINTER(C.c_double)
    L = C.CDLL(LS._build(os.path.join(out_dir, "libprojection_product.so"), deps, cmd))
    L.product_latlong_rays.argtypes = [dp, dp, C.c_longlong, dp, dp]
    _PRODUCT = L
    return L


def product_latlong_rays(origin, rotation, cxcy):
    dp = C.POINTER(C.c_double)
    o, R, cxcy = LS.f64(origin).reshape(3), LS.f64(rotation).reshape(9), LS.f64(cxcy).reshape(-1, 2)
    out = np.zeros((len(cxcy), 6))
    product().product_latlong_rays(o.ctypes.data_as(dp), R.ctypes.data_as(dp), len(cxcy), cxcy.ctypes.data_as(dp), out.ctypes.data_as(dp))
    return out[:, :3], out[:, 3:]
