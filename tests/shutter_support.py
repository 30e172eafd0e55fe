"""Shared by the camera-shutter tests: builds and loads the restatement tests/c/shutter_oracle.c (rays_oracle.c and everything under it
included unchanged, plus the shutter ray written out in C from include/ptx.h), compiles the product's own rule (csrc/pt_shutter.h) for
the host, and holds the camera states and samples the CPU and GPU tests share.

Both libraries are compiled into build/ (out of git).  The restatement carries its own copy of the oracle's globals, so its math mode
is set here, to the shared pt_math.h functions (0), before anything is compared with the GPU.
"""
import ctypes as C
import os

import numpy as np

import camera_pose_support as CS
import lens_support as LS
from camera_pose_support import Pose, cam4_of, rotation  # noqa: F401
from lens_support import ImageRecord, bits, f64, i32, pass_order_sums  # noqa: F401
from path_tracer_ocaml_amd import abi

ROOT = LS.ROOT
dp, ip = abi.c_double_p, abi.c_int32_p
_LIB = None
_PRODUCT = None
W, H, SPP = 13, 11, 4  # two tile columns and two tile rows, both ragged
DEPTHS = (0, 1, 4)
CASES = LS.CASES
IDENTITY, ZERO = np.eye(3), np.zeros(3)


def _dp(a):
    return None if a is None else a.ctypes.data_as(dp)


def all_samples(width=W, height=H, spp=SPP):
    """every (x, y, pass) of a frame, pixel-major (lens_support's, at this module's frame)"""
    return LS.all_samples(width, height, spp)


def _ip(a):
    return a.ctypes.data_as(ip)


def lib():
    global _LIB
    if _LIB is not None:
        return _LIB
    c = os.path.join(ROOT, "tests", "c")
    src = os.path.join(c, "shutter_oracle.c")
    deps = [src] + [os.path.join(c, f) for f in ("rays_oracle.c", "camera_pose_oracle.c", "lens_oracle.c", "envlight_oracle.c", "texture_oracle.c")] + \
        [os.path.join(ROOT, "oracle", "pt_oracle.c"), os.path.join(ROOT, "include", "ptx.h"),
         os.path.join(ROOT, "path_tracer_ocaml_amd", "csrc", "pt_math.h")]
    so = LS._build(os.path.join(ROOT, "build", "libshutter_oracle.so"), deps,
                   lambda tmp: [os.environ.get("CC", "gcc"), *LS._oracle_cflags(), "-shared", "-o", tmp, src, "-lm", "-lpthread"])
    L = C.CDLL(so)
    L.orc_set_math.argtypes = [C.c_int]
    L.orc_scene_create.restype = C.c_void_p
    L.orc_scene_create.argtypes = [C.POINTER(abi.SceneDesc)]
    L.orc_scene_destroy.argtypes = [C.c_void_p]
    camera = [dp, dp, dp, C.c_double, C.c_double, C.c_int, dp, dp, C.c_double]  # o, R, view4, A, F, latlong, T, k, angle
    frame = [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int64, ip, ip, ip]  # width, height, spp, max_bounces, n, xs, ys, passes
    L.orcs_sample_rays.argtypes = [C.c_void_p, *camera, *frame, dp]
    L.orcs_trace_samples.restype = C.c_int
    L.orcs_trace_samples.argtypes = [C.c_void_p, C.POINTER(ImageRecord), dp, C.c_int, C.c_int, C.c_int, dp, C.c_int, C.c_int, *camera, *frame, dp,
                                     C.POINTER(C.c_int64)]
    L.orcr_first_hits.argtypes = [C.c_void_p, C.POINTER(ImageRecord), dp, C.c_int, C.c_int, C.c_int, dp, C.c_int64, dp, dp]
    L.orc_set_math(0)
    _LIB = L
    return L


_PRODUCT_SRC = """
#include "pt_shutter.h"
/* kind: 0 the posed camera, 1 through a lens, 2 the lat-long panorama.  shutter == 0: the rule WITHOUT a shutter on the same inputs
 * (pt_camera_pose_ray / pt_latlong_ray). */
extern "C" void product_shutter_rays(const double* cam4, const double* o, const double* R, const double* T, const double* k, double angle,
                                     int kind, int shutter, double radius, double F, long long n, const double* cxcy, const double* uv,
                                     const double* t, double* out) {
  PtCameraPose cp;
  PtShutter sh;
  for (int i = 0; i < 3; ++i) { cp.o[i] = o[i]; sh.tr[i] = T[i]; sh.k[i] = k[i]; }
  for (int i = 0; i < 9; ++i) cp.r[i] = R[i];
  cp.llx = cam4[0]; cp.lly = cam4[1]; cp.vx = cam4[2]; cp.vy = cam4[3];
  sh.angle = angle;
  sh.dim = 0; /* (the rule does not read it) */
  for (long long i = 0; i < n; ++i) {
    V3 ro, rd;
    const double cx = cxcy[2 * i], cy = cxcy[2 * i + 1], u = uv[2 * i], v = uv[2 * i + 1];
    if (shutter) {
      if (kind == 2) pt_shutter_latlong_ray(cp, sh, cx, cy, t[i], &ro, &rd);
      else if (kind == 1) pt_shutter_pose_ray<true>(cp, sh, cx, cy, radius, F, u, v, t[i], &ro, &rd);
      else pt_shutter_pose_ray<false>(cp, sh, cx, cy, 0.0, 1.0, 0.0, 0.0, t[i], &ro, &rd);
    } else {
      if (kind == 2) pt_latlong_ray(cp, cx, cy, &ro, &rd);
      else if (kind == 1) pt_camera_pose_ray<true>(cp, cx, cy, radius, F, u, v, &ro, &rd);
      else pt_camera_pose_ray<false>(cp, cx, cy, 0.0, 1.0, 0.0, 0.0, &ro, &rd);
    }
    out[6 * i] = ro.x; out[6 * i + 1] = ro.y; out[6 * i + 2] = ro.z; out[6 * i + 3] = rd.x; out[6 * i + 4] = rd.y; out[6 * i + 5] = rd.z;
  }
}
"""


def product():
    """csrc/pt_shutter.h -- the functions the kernels call -- compiled for the host with the library's floating-point flags"""
    global _PRODUCT
    if _PRODUCT is not None:
        return _PRODUCT
    csrc = os.path.join(ROOT, "path_tracer_ocaml_amd", "csrc")
    deps = [os.path.join(csrc, f) for f in ("pt_shutter.h", "pt_projection.h", "pt_camera_pose.h", "pt_vec.h", "pt_math.h")] + [os.path.abspath(__file__)]
    out_dir = os.path.join(ROOT, "build")
    os.makedirs(out_dir, exist_ok=True)
    src = os.path.join(out_dir, "shutter_product.cpp")

    def cmd(tmp):
        with open(src, "w") as f:
            f.write(_PRODUCT_SRC)
        return [os.environ.get("CXX", "g++"), "-std=c++17", "-O2", "-fPIC", "-ffp-contract=off", "-fno-fast-math", "-march=x86-64-v3",
                "-I", csrc, "-shared", "-o", tmp, src]
    L = C.CDLL(LS._build(os.path.join(out_dir, "libshutter_product.so"), deps, cmd))
    L.product_shutter_rays.argtypes = [dp, dp, dp, dp, dp, C.c_double, C.c_int, C.c_int, C.c_double, C.c_double, C.c_longlong, dp, dp, dp, dp]
    _PRODUCT = L
    return L


KINDS = {"pose": 0, "lens": 1, "latlong": 2}


def product_rays(kind, cam4, origin, rotation_, T, k, angle, cxcy, t, lens=None, uv=None, shutter=True):
    """(n, 6) rays from csrc/pt_shutter.h (shutter=False: from the posed / lat-long rule on the same inputs)"""
    cam4, o, R, T, k = f64(cam4), f64(origin).reshape(3), f64(rotation_).reshape(9), f64(T).reshape(3), f64(k).reshape(3)
    cxcy = f64(cxcy).reshape(-1, 2)
    n = len(cxcy)
    uv = f64(np.zeros_like(cxcy) if uv is None else uv).reshape(-1, 2)
    t = f64(np.broadcast_to(np.asarray(t, dtype=np.float64), (n,)))
    radius, F = (0.0, 1.0) if lens is None else (float(lens[0]), float(lens[1]))
    out = np.zeros((n, 6))
    product().product_shutter_rays(_dp(cam4), _dp(o), _dp(R), _dp(T), _dp(k), float(angle), KINDS[kind], int(shutter), radius, F, n, _dp(cxcy),
                                   _dp(uv), _dp(t), _dp(out))
    return out


class State:
    """A handle's camera state: a pose (camera_pose_support.Pose, or None: off), a lens (bool: the case's), the projection and the
    shutter (T, k, A), or None: off"""

    def __init__(self, pose=None, lens=False, latlong=False, shutter=None):
        self.pose, self.lens, self.latlong = pose, lens, latlong
        self.shutter = None if shutter is None else (f64(shutter[0]).reshape(3), f64(shutter[1]).reshape(3), float(shutter[2]))

    def set_on(self, g, c):
        """in an order the setters accept from any earlier state of these tests"""
        g.set_lens(0.0, 1.0)
        g.set_camera_projection("latlong" if self.latlong else "perspective")
        if self.lens:
            g.set_lens(*c["lens"])
        if self.pose is None:
            g.set_camera_pose()
        else:
            self.pose.set_on(g)
        if self.shutter is None:
            g.set_camera_shutter()
        else:
            g.set_camera_shutter(*self.shutter)

    def c_args(self, c):
        """orcs_*'s camera arguments, and what keeps them alive"""
        pose = self.pose or Pose()
        o, R, v = pose.c_args()
        A, F = c["lens"] if self.lens else (0.0, 1.0)
        T, k, angle = self.shutter
        keep = (o, R, v, T, k)
        return (_dp(o), _dp(R), _dp(v), float(A), float(F), int(self.latlong), _dp(T), _dp(k), angle), keep


class Restatement:
    """A scene of the restatement library for a ptx_scene_desc pointer."""

    def __init__(self, desc_ptr, keepalive=None):
        self._keep = keepalive
        self._h = lib().orc_scene_create(desc_ptr)
        assert self._h
        self._n_textures = desc_ptr.contents.n_textures

    _table = LS.Restatement._table
    _env = staticmethod(LS.Restatement._env)

    def rays(self, c, state, width, height, spp, max_bounces, xs, ys, passes):
        xs, ys, passes = i32(xs), i32(ys), i32(passes)
        rays = np.zeros((len(xs), 6))
        cam, keep = state.c_args(c)
        lib().orcs_sample_rays(self._h, *cam, width, height, spp, max_bounces, len(xs), _ip(xs), _ip(ys), _ip(passes), _dp(rays))
        del keep
        return rays

    def trace_samples(self, c, state, width, height, spp, max_bounces, xs, ys, passes, mode=0):
        """(radiance n x 3, segments)"""
        xs, ys, passes = i32(xs), i32(ys), i32(passes)
        table, keep = self._table(c["images"])
        e = self._env(c["env"])
        rgb, seg = np.zeros((len(xs), 3)), C.c_int64(0)
        cam, keep2 = state.c_args(c)
        rc = lib().orcs_trace_samples(self._h, table, *e[:5], mode, int(c["sampling"]), *cam, width, height, spp, max_bounces, len(xs), _ip(xs),
                                      _ip(ys), _ip(passes), _dp(rgb), C.byref(seg))
        assert rc == 0, rc
        del keep, keep2
        return rgb, seg.value

    def first_hits(self, c, state, width, height, spp, max_bounces, xs, ys, passes):
        """the feature records (n x 8) of the samples' shutter rays"""
        rays = self.rays(c, state, width, height, spp, max_bounces, xs, ys, passes)
        table, keep = self._table(c["images"])
        e = self._env(c["env"])
        feat = np.zeros((len(rays), 8))
        lib().orcr_first_hits(self._h, table, *e[:5], len(rays), _dp(rays), _dp(feat))
        del keep
        return feat

    def close(self):
        if self._h:
            lib().orc_scene_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


# ------------------------------------------------------------------------------------------------ the cases CPU and GPU tests share
_CACHE = {}
AXIS = np.array([0.2, 0.9, -0.3]) / np.linalg.norm([0.2, 0.9, -0.3])  # off every coordinate axis, signs mixed


def case(name, oracle, width=W, height=H):
    """camera_pose_support's case with this library's restatement ("sref") and the camera states of the shutter tests.  The motion is
    scaled to the scene like the case's poses: a twentieth of the focus distance, and a turn of 0.12 rad about a skew axis.
      both      the oblique pose, a shutter that translates and turns          turn      the oblique pose, a pure turn
      move      the oblique pose, a pure translation                          pose_off  the same shutter with the pose off
      lens      the oblique pose through the case's lens                       latlong   the panorama from the oblique pose"""
    key = (name, width, height)
    if key in _CACHE:
        return _CACHE[key]
    c = dict(CS.case(name, oracle, width, height))
    c["sref"] = Restatement(c["desc"], c["keep"])
    F = c["lens"][1]
    T = 0.05 * F * np.array([0.6, 0.3, -0.7])
    oblique = c["poses"]["oblique"]
    c["states"] = {"both": State(oblique, shutter=(T, AXIS, 0.12)),
                   "turn": State(oblique, shutter=(ZERO, AXIS, -0.12)),
                   "move": State(oblique, shutter=(T, ZERO, 0.0)),
                   "pose_off": State(None, shutter=(T, AXIS, 0.12)),
                   "lens": State(oblique, lens=True, shutter=(T, AXIS, 0.12)),
                   "latlong": State(oblique, latlong=True, shutter=(T, AXIS, 0.12))}
    _CACHE[key] = c
    return c


def gpu_scene(P, c, state, mode=0):
    """the GPU scene of a case under a camera state (None: the scene's own camera)"""
    g = LS.gpu_scene(P, c, mode, lens=False)
    if state is not None:
        state.set_on(g, c)
    return g


def restated(c, state, depth, mode=0, width=W, height=H, spp=SPP, samples=None):
    """the restatement's (radiance, segments) for all samples of the frame (or `samples`), under the case's shading state"""
    xs, ys, ps = samples if samples is not None else all_samples(width, height, spp)
    return c["sref"].trace_samples(c, state, width, height, spp, depth, xs, ys, ps, mode)


def numpy_rays(oracle, c, state, width, height, spp, depth, xs, ys, passes, t=None):
    """the numpy rule on film coordinates, lens pairs and times restated from the sampler (t given: the caller's times instead)"""
    import shutter_reference as SR
    lens = c["lens"] if state.lens else None
    d = SR.dimension(depth, lens)
    xs, ys, passes = (np.asarray(a, dtype=np.int64) for a in (xs, ys, passes))
    off = ys * width + xs + passes * spp
    get = lambda j: oracle.lds_get_vec(d, off, np.full(len(off), j))  # noqa: E731
    cx = (xs.astype(np.float64) + get(0)) * (1.0 / np.float64(width))
    cy = 1.0 - ((ys.astype(np.float64) + get(1)) * (1.0 / np.float64(height)))
    uv = np.stack([get(d - 3), get(d - 2)], axis=1) if lens else None
    if t is None:
        t = get(d - 1)
    pose = state.pose or Pose()
    view = pose.view or cam4_of(c["desc"])
    T, k, A = state.shutter
    o, dirs = SR.shutter_rays(view, pose.origin, pose.rotation, T, k, A, np.stack([cx, cy], axis=1), t, lens, uv, state.latlong)
    return np.concatenate([o, dirs], axis=1)
