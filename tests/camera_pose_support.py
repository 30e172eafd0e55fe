"""Shared by the camera-pose tests: builds and loads the restatement tests/c/camera_pose_oracle.c (lens_oracle.c and everything under
it included unchanged, plus the posed ray written out in C from include/ptx.h), compiles the product's own rule
(csrc/pt_camera_pose.h) for the host, and holds the scenes, poses and samples the CPU and GPU tests share.

Both libraries are compiled into build/ (out of git).  The restatement carries its own copy of the oracle's globals, so its math mode
is set here, to the shared pt_math.h functions (0), before anything is compared with the GPU.
"""
import ctypes as C
import os

import numpy as np

import lens_support as LS
from lens_support import ImageRecord, all_samples, bits, f64, i32, pass_order_sums  # noqa: F401
from path_tracer_ocaml_amd import abi

ROOT = LS.ROOT
dp, ip = abi.c_double_p, abi.c_int32_p
_LIB = None
_PRODUCT = None
W, H, SPP = LS.W, LS.H, LS.SPP
DEPTHS = (0, 1, 8)
CASES = LS.CASES
IDENTITY = np.eye(3)
ZERO = np.zeros(3)


def _dp(a):
    return None if a is None else a.ctypes.data_as(dp)


def _ip(a):
    return a.ctypes.data_as(ip)


def lib():
    global _LIB
    if _LIB is not None:
        return _LIB
    c = os.path.join(ROOT, "tests", "c")
    src = os.path.join(c, "camera_pose_oracle.c")
    deps = [src, os.path.join(c, "lens_oracle.c"), os.path.join(c, "envlight_oracle.c"), os.path.join(c, "texture_oracle.c"),
            os.path.join(ROOT, "oracle", "pt_oracle.c"), os.path.join(ROOT, "include", "ptx.h"),
            os.path.join(ROOT, "path_tracer_ocaml_amd", "csrc", "pt_math.h")]
    so = LS._build(os.path.join(ROOT, "build", "libcamera_pose_oracle.so"), deps,
                   lambda tmp: [os.environ.get("CC", "gcc"), *LS._oracle_cflags(), "-shared", "-o", tmp, src, "-lm", "-lpthread"])
    L = C.CDLL(so)
    L.orc_set_math.argtypes = [C.c_int]
    L.orc_scene_create.restype = C.c_void_p
    L.orc_scene_create.argtypes = [C.POINTER(abi.SceneDesc)]
    L.orc_scene_destroy.argtypes = [C.c_void_p]
    L.orcn_sample_rays.argtypes = [C.c_void_p, C.c_double, C.c_double, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int64, ip, ip, ip,
                                   dp, dp]
    L.orcn_trace_samples.argtypes = [C.c_void_p, C.POINTER(ImageRecord), dp, C.c_int, C.c_int, C.c_int, dp, C.c_int, C.c_int, C.c_double,
                                     C.c_double, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int64, ip, ip, ip, dp,
                                     C.POINTER(C.c_int64)]
    L.orcp_pose_rays.argtypes = [dp, dp, dp, C.c_double, C.c_double, C.c_int64, dp, dp, dp]
    L.orcp_sample_rays.argtypes = [C.c_void_p, dp, dp, dp, C.c_double, C.c_double, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int64, ip, ip, ip, dp]
    L.orcp_trace_samples.argtypes = [C.c_void_p, C.POINTER(ImageRecord), dp, C.c_int, C.c_int, C.c_int, dp, C.c_int, C.c_int, dp, dp, dp,
                                     C.c_double, C.c_double, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int64, ip, ip, ip, dp, C.POINTER(C.c_int64)]
    L.orcp_first_hits.argtypes = [C.c_void_p, C.POINTER(ImageRecord), dp, C.c_int, C.c_int, C.c_int, dp, dp, dp, dp, C.c_double, C.c_double,
                                  C.c_int, C.c_int, C.c_int, C.c_int, C.c_int64, ip, ip, ip, dp]
    L.orc_set_math(0)
    _LIB = L
    return L


_PRODUCT_SRC = """
#include "pt_camera_pose.h"
extern "C" void product_pose_rays(const double* cam4, const double* o, const double* R, int lens, double A, double F, long long n,
                                  const double* cxcy, const double* uv, double* out) {
  PtCameraPose cp;
  for (int i = 0; i < 3; ++i) cp.o[i] = o[i];
  for (int i = 0; i < 9; ++i) cp.r[i] = R[i];
  cp.llx = cam4[0]; cp.lly = cam4[1]; cp.vx = cam4[2]; cp.vy = cam4[3];
  for (long long i = 0; i < n; ++i) {
    V3 ro, rd;
    if (lens) pt_camera_pose_ray<true>(cp, cxcy[2 * i], cxcy[2 * i + 1], A, F, uv[2 * i], uv[2 * i + 1], &ro, &rd);
    else pt_camera_pose_ray<false>(cp, cxcy[2 * i], cxcy[2 * i + 1], 0.0, 1.0, 0.0, 0.0, &ro, &rd);
    out[6 * i] = ro.x; out[6 * i + 1] = ro.y; out[6 * i + 2] = ro.z; out[6 * i + 3] = rd.x; out[6 * i + 4] = rd.y; out[6 * i + 5] = rd.z;
  }
}
"""


def product():
    """csrc/pt_camera_pose.h -- the function the kernels call -- compiled for the host with the library's floating-point flags"""
    global _PRODUCT
    if _PRODUCT is not None:
        return _PRODUCT
    csrc = os.path.join(ROOT, "path_tracer_ocaml_amd", "csrc")
    deps = [os.path.join(csrc, f) for f in ("pt_camera_pose.h", "pt_vec.h", "pt_math.h")] + [os.path.abspath(__file__)]
    out_dir = os.path.join(ROOT, "build")
    os.makedirs(out_dir, exist_ok=True)
    src = os.path.join(out_dir, "camera_pose_product.cpp")

    def cmd(tmp):
        with open(src, "w") as f:
            f.write(_PRODUCT_SRC)
        return [os.environ.get("CXX", "g++"), "-std=c++17", "-O2", "-fPIC", "-ffp-contract=off", "-fno-fast-math", "-march=x86-64-v3",
                "-I", csrc, "-shared", "-o", tmp, src]
    L = C.CDLL(LS._build(os.path.join(out_dir, "libcamera_pose_product.so"), deps, cmd))
    L.product_pose_rays.argtypes = [dp, dp, dp, C.c_int, C.c_double, C.c_double, C.c_longlong, dp, dp, dp]
    _PRODUCT = L
    return L


def _lens_args(lens):
    return (0.0, 1.0) if lens is None else (float(lens[0]), float(lens[1]))


def c_pose_rays(cam4, origin, rotation, cxcy, lens=None, uv=None):
    cam4, o, R, cxcy = f64(cam4), f64(origin).reshape(3), f64(rotation).reshape(9), f64(cxcy).reshape(-1, 2)
    uv = f64(np.zeros_like(cxcy) if uv is None else uv).reshape(-1, 2)
    out = np.zeros((len(cxcy), 6))
    lib().orcp_pose_rays(_dp(cam4), _dp(o), _dp(R), *_lens_args(lens), len(cxcy), _dp(cxcy), _dp(uv), _dp(out))
    return out


def product_pose_rays(cam4, origin, rotation, cxcy, lens=None, uv=None):
    cam4, o, R, cxcy = f64(cam4), f64(origin).reshape(3), f64(rotation).reshape(9), f64(cxcy).reshape(-1, 2)
    uv = f64(np.zeros_like(cxcy) if uv is None else uv).reshape(-1, 2)
    out = np.zeros((len(cxcy), 6))
    product().product_pose_rays(_dp(cam4), _dp(o), _dp(R), int(lens is not None), *_lens_args(lens), len(cxcy), _dp(cxcy), _dp(uv), _dp(out))
    return out


def rotation(axis, angle):
    """Rodrigues: the rotation by `angle` about `axis` (orthonormal to a few ulps: far inside the setter's 1e-9)"""
    a = np.asarray(axis, dtype=np.float64)
    a = a / np.linalg.norm(a)
    K = np.array([[0.0, -a[2], a[1]], [a[2], 0.0, -a[0]], [-a[1], a[0], 0.0]])
    return np.eye(3) + np.sin(angle) * K + (1.0 - np.cos(angle)) * (K @ K)


class Pose:
    """(origin, rotation, view or None) as the setter takes them"""

    def __init__(self, origin=None, rotation=None, view=None):
        self.given = origin is not None
        self.origin = ZERO.copy() if origin is None else f64(origin).reshape(3)
        self.rotation = IDENTITY.copy() if rotation is None else f64(rotation).reshape(3, 3)
        self.view = None if view is None else tuple(float(v) for v in view)

    def set_on(self, g):
        g.set_camera_pose(self.origin if self.given else None, self.rotation if self.given else None, self.view)

    def c_args(self):
        keep = (f64(self.origin), f64(self.rotation).reshape(9), None if self.view is None else f64(self.view))
        return keep


class Restatement:
    """A scene of the restatement library for a ptx_scene_desc pointer."""

    def __init__(self, desc_ptr, keepalive=None):
        self._keep = keepalive
        self._h = lib().orc_scene_create(desc_ptr)
        assert self._h
        self._n_textures = desc_ptr.contents.n_textures

    _table = LS.Restatement._table
    _env = staticmethod(LS.Restatement._env)

    def rays(self, pose, width, height, spp, max_bounces, xs, ys, passes, lens=None):
        """rays n x 6 of the samples' camera rays; pose None: the scene's own camera (orcn_sample_rays: the pinhole, or the lens)"""
        xs, ys, passes = i32(xs), i32(ys), i32(passes)
        rays = np.zeros((len(xs), 6))
        if pose is None:
            lib().orcn_sample_rays(self._h, *_lens_args(lens), 0, width, height, spp, max_bounces, len(xs), _ip(xs), _ip(ys), _ip(passes),
                                   _dp(rays), None)
            return rays
        o, R, v = pose.c_args()
        lib().orcp_sample_rays(self._h, _dp(o), _dp(R), _dp(v), *_lens_args(lens), width, height, spp, max_bounces, len(xs), _ip(xs), _ip(ys),
                               _ip(passes), _dp(rays))
        return rays

    def trace_samples(self, pose, width, height, spp, max_bounces, xs, ys, passes, images=None, env=None, mode=0, sampling=False, lens=None):
        """(radiance n x 3, segments); pose None: the scene's own camera"""
        xs, ys, passes = i32(xs), i32(ys), i32(passes)
        table, keep = self._table(images)
        e = self._env(env)
        rgb, seg = np.zeros((len(xs), 3)), C.c_int64(0)
        if pose is None:
            rc = lib().orcn_trace_samples(self._h, table, *e[:5], mode, int(sampling), *_lens_args(lens), 0, width, height, spp, max_bounces,
                                          len(xs), _ip(xs), _ip(ys), _ip(passes), _dp(rgb), C.byref(seg))
        else:
            o, R, v = pose.c_args()
            rc = lib().orcp_trace_samples(self._h, table, *e[:5], mode, int(sampling), _dp(o), _dp(R), _dp(v), *_lens_args(lens), width, height,
                                          spp, max_bounces, len(xs), _ip(xs), _ip(ys), _ip(passes), _dp(rgb), C.byref(seg))
        assert rc == 0, rc
        del keep
        return rgb, seg.value

    def first_hits(self, pose, width, height, spp, max_bounces, xs, ys, passes, images=None, env=None, lens=None):
        """the feature records (n x 8) of the samples' posed camera rays"""
        xs, ys, passes = i32(xs), i32(ys), i32(passes)
        table, keep = self._table(images)
        e = self._env(env)
        feat = np.zeros((len(xs), 8))
        o, R, v = pose.c_args()
        lib().orcp_first_hits(self._h, table, *e[:5], _dp(o), _dp(R), _dp(v), *_lens_args(lens), width, height, spp, max_bounces, len(xs),
                              _ip(xs), _ip(ys), _ip(passes), _dp(feat))
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
OBLIQUE_R = rotation((0.3, 1.0, 2.0), 0.15)  # mostly a roll, so the scene stays in view; every entry non-zero, signs mixed


def cam4_of(desc_ptr):
    cam = desc_ptr.contents.camera
    return (cam.lower_left_x, cam.lower_left_y, cam.view_x, cam.view_y)


def _spheres(desc_ptr):
    d = desc_ptr.contents
    n = d.n_spheres
    if n == 0:
        return np.zeros((0, 4)), np.zeros(0, dtype=np.int32)
    arr = lambda p, dt: np.ctypeslib.as_array(p, shape=(n,)).astype(dt)  # noqa: E731
    xyzr = np.stack([arr(d.sphere_x, np.float64), arr(d.sphere_y, np.float64), arr(d.sphere_z, np.float64), arr(d.sphere_r, np.float64)], axis=1)
    kinds = np.array([d.materials[int(m)].kind for m in arr(d.sphere_material, np.int32)], dtype=np.int32)
    return xyzr, kinds


def case(name, oracle, width=W, height=H):
    """lens_support's case (descriptor, images, environment, its lens) with this library's restatement and the case's poses:
      oblique        off the scene's own eye by a tenth of the case's focus distance, turned about a skew axis
      view           a view override alone (origin 0, the identity): another aspect, off centre
      inside_glass   (scenes with a large glass sphere) the origin INSIDE it: the first hit is from inside
      below_ground   (scenes on a ground sphere) the origin below the ground's surface, under the scene's own eye"""
    key = (name, width, height)
    if key in _CACHE:
        return _CACHE[key]
    c = dict(LS.case(name, oracle, width, height))
    c["ref"] = Restatement(c["desc"], c["keep"])
    llx, lly, vx, vy = cam4_of(c["desc"])
    F = c["lens"][1]
    poses = {"oblique": Pose(0.1 * F * np.array([0.3, -0.2, 0.5]), OBLIQUE_R),
             "view": Pose(view=(0.7 * llx, 1.25 * lly, 0.6 * vx * 1.5, 1.25 * vy * 0.9))}
    xyzr, kinds = _spheres(c["desc"])
    glass = [i for i in range(len(kinds)) if kinds[i] == abi.PTX_MAT_DIELECTRIC and xyzr[i, 3] < 100.0]
    if glass:
        g = xyzr[max(glass, key=lambda i: xyzr[i, 3])]
        poses["inside_glass"] = Pose(g[:3] + 0.3 * g[3] * np.array([0.5, 0.5, -0.7]), rotation((0.2, 1.0, 0.1), -0.9))
    ground = [i for i in range(len(kinds)) if xyzr[i, 3] >= 100.0]
    if ground:
        s = xyzr[ground[0]]
        up = -s[:3] / np.linalg.norm(s[:3])  # from the ground's centre to the scene's own eye
        poses["below_ground"] = Pose(s[:3] + (s[3] - 0.5) * up, rotation((1.0, 0.3, 0.2), 0.7))
    c["poses"] = poses
    _CACHE[key] = c
    return c


def gpu_scene(P, c, pose, mode=0, lens=False):
    """the GPU scene of a case under a pose (None: off)"""
    g = LS.gpu_scene(P, c, mode, lens=lens)
    if pose is not None:
        pose.set_on(g)
    return g


def restated(c, pose, depth, mode=0, lens=False, width=W, height=H, spp=SPP, samples=None):
    """the restatement's (radiance, segments) for all samples of the frame (or `samples`), under the case's state"""
    xs, ys, ps = samples if samples is not None else all_samples(width, height, spp)
    return c["ref"].trace_samples(pose, width, height, spp, depth, xs, ys, ps, c["images"], c["env"], mode, c["sampling"],
                                  c["lens"] if lens else None)
