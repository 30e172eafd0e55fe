"""Shared by the ray-entry-point tests (ptx_render_rays): builds and loads the restatement tests/c/rays_oracle.c (camera_pose_oracle.c
and everything under it included unchanged, plus the path loop on explicit (ray, offset) pairs), and makes the ray families the CPU
and GPU tests share.

The library is compiled into build/ (out of git).  It carries its own copy of the oracle's globals, so its math mode is set here, to
the shared pt_math.h functions (0), before anything is compared with the GPU.
"""
import ctypes as C
import os

import numpy as np

import camera_pose_support as CS
import lens_support as LS
from lens_support import ImageRecord, all_samples, bits, f64, i32  # noqa: F401
from path_tracer_ocaml_amd import abi

ROOT = LS.ROOT
dp, ip = abi.c_double_p, abi.c_int32_p
_LIB = None
W, H, SPP = LS.W, LS.H, LS.SPP
N = W * H
DEPTHS = LS.DEPTHS  # (0, 1, 4)
CASES = LS.CASES
MUTANTS = {"bounce dimensions from 0": 1}
MAX_OFFSET = 2**31 - 2


def lib():
    global _LIB
    if _LIB is not None:
        return _LIB
    c = os.path.join(ROOT, "tests", "c")
    src = os.path.join(c, "rays_oracle.c")
    deps = [src] + [os.path.join(c, f) for f in ("camera_pose_oracle.c", "lens_oracle.c", "envlight_oracle.c", "texture_oracle.c")] + \
        [os.path.join(ROOT, "oracle", "pt_oracle.c"), os.path.join(ROOT, "include", "ptx.h"),
         os.path.join(ROOT, "path_tracer_ocaml_amd", "csrc", "pt_math.h")]
    so = LS._build(os.path.join(ROOT, "build", "librays_oracle.so"), deps,
                   lambda tmp: [os.environ.get("CC", "gcc"), *LS._oracle_cflags(), "-shared", "-o", tmp, src, "-lm", "-lpthread"])
    L = C.CDLL(so)
    L.orc_set_math.argtypes = [C.c_int]
    L.orc_scene_create.restype = C.c_void_p
    L.orc_scene_create.argtypes = [C.POINTER(abi.SceneDesc)]
    L.orc_scene_destroy.argtypes = [C.c_void_p]
    L.orcr_trace_rays.argtypes = [C.c_void_p, C.POINTER(ImageRecord), dp, C.c_int, C.c_int, C.c_int, dp, C.c_int, C.c_int, C.c_int, C.c_int,
                                  C.c_int, C.c_int, C.c_int64, dp, ip, dp, C.POINTER(C.c_int64)]
    L.orcr_first_hits.argtypes = [C.c_void_p, C.POINTER(ImageRecord), dp, C.c_int, C.c_int, C.c_int, dp, C.c_int64, dp, dp]
    L.orc_set_math(0)
    _LIB = L
    return L


def sampler_dim(max_bounces, lens=False):
    return 2 + 2 * max_bounces + (2 if lens else 0)


class Restatement:
    """A scene of this library for a ptx_scene_desc pointer."""

    def __init__(self, desc_ptr, keepalive=None):
        self._keep = keepalive
        self._h = lib().orc_scene_create(desc_ptr)
        assert self._h
        self._n_textures = desc_ptr.contents.n_textures

    _table = LS.Restatement._table
    _env = staticmethod(LS.Restatement._env)

    def trace_rays(self, rays, offsets, max_bounces, dim=None, images=None, env=None, mode=0, sampling=False, normalize=False, mutant=0):
        """(radiance n x 3, segments) of rays n x 6 at the offsets (None: i)"""
        rays = f64(rays).reshape(-1, 6)
        off = None if offsets is None else i32(offsets)
        table, keep = self._table(images)
        e = self._env(env)
        rgb, seg = np.zeros((len(rays), 3)), C.c_int64(0)
        rc = lib().orcr_trace_rays(self._h, table, *e[:5], mode, int(sampling), sampler_dim(max_bounces) if dim is None else dim,
                                   int(normalize), mutant, max_bounces, len(rays), rays.ctypes.data_as(dp),
                                   None if off is None else off.ctypes.data_as(ip), rgb.ctypes.data_as(dp), C.byref(seg))
        assert rc == 0, rc
        del keep
        return rgb, seg.value

    def first_hits(self, rays, images=None, env=None):
        """the feature records (n x 8) of rays n x 6"""
        rays = f64(rays).reshape(-1, 6)
        table, keep = self._table(images)
        e = self._env(env)
        feat = np.zeros((len(rays), 8))
        lib().orcr_first_hits(self._h, table, *e[:5], len(rays), rays.ctypes.data_as(dp), feat.ctypes.data_as(dp))
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


_CACHE = {}


def case(name, oracle):
    """camera_pose_support's case with this library's restatement under "rays_ref" """
    if name in _CACHE:
        return _CACHE[name]
    c = dict(CS.case(name, oracle))
    c["rays_ref"] = Restatement(c["desc"], c["keep"])
    _CACHE[name] = c
    return c


def frame_offsets(width=W, height=H, spp=SPP):
    """the sampler offsets y W + x + pass N of all_samples' (x, y, pass)"""
    xs, ys, ps = all_samples(width, height, spp)
    return i32(ys.astype(np.int64) * width + xs + ps.astype(np.int64) * spp)


def _cosine_dirs(normals, rng):
    """cosine-weighted directions about unit normals (any orthonormal frame: the test only needs plausible rays)"""
    n = normals / np.linalg.norm(normals, axis=1, keepdims=True)
    a = np.where(np.abs(n[:, :1]) < 0.9, np.array([[1.0, 0.0, 0.0]]), np.array([[0.0, 1.0, 0.0]]))
    t = np.cross(n, a)
    t /= np.linalg.norm(t, axis=1, keepdims=True)
    b = np.cross(n, t)
    u, v = rng.random(len(n)), rng.random(len(n))
    r, phi = np.sqrt(u), 2.0 * np.pi * v
    d = (r * np.cos(phi))[:, None] * t + (r * np.sin(phi))[:, None] * b + np.sqrt(1.0 - u)[:, None] * n
    return d / np.linalg.norm(d, axis=1, keepdims=True)


def ray_families(c, seed=7):
    """About 250 rays of a case, {"rays": n x 6, "offsets": n, "scaled": n x 6} -- unit directions in "rays"; "scaled" holds the same
    origins with directions of length 1e-3 .. 1e3 (for PTX_RAYS_NORMALIZE).  Families:
      camera      the case's own camera rays (every sixth sample)
      surface     origins at the restatement's first hits pushed 1e-3 along the normal, cosine directions
      placed      origins inside the glass sphere, below the ground and outside the tree's box, aimed at the scene and away from it
      axis        axis-parallel directions with +0 and -0 components
    Offsets: 0, i, repeated values and 2^31 - 2, mixed over the rays."""
    rng = np.random.default_rng(seed)
    xs, ys, ps = all_samples()
    pick = np.arange(0, len(xs), 6)
    cam = c["ref"].rays(None, W, H, SPP, 4, xs[pick], ys[pick], ps[pick])
    feat = c["ref"].first_hits(CS.Pose(CS.ZERO, CS.IDENTITY), W, H, SPP, 4, xs[pick], ys[pick], ps[pick], c["images"], c["env"])
    hit = feat[:, 7] > 0
    points = cam[hit, :3] + feat[hit, 6:7] * cam[hit, 3:] + 1e-3 * feat[hit, 3:6]
    surface = np.concatenate([points, _cosine_dirs(feat[hit, 3:6], rng)], axis=1)
    centre = points.mean(axis=0) if hit.any() else np.array([0.0, 0.0, -5.0])
    origins = [p.origin for p in c["poses"].values() if p.given]
    origins.append(centre + np.array([0.0, 4000.0, 0.0]))   # far outside every tree's box
    origins.append(centre + np.array([-3000.0, 10.0, 2500.0]))
    placed = []
    for o in origins:
        to = (centre - o) / max(np.linalg.norm(centre - o), 1e-12)
        for _ in range(8):
            d = to + 0.3 * rng.standard_normal(3)
            d /= np.linalg.norm(d)
            placed.append(np.concatenate([o, d]))
            placed.append(np.concatenate([o, -d]))
    placed = np.array(placed)
    axis = []
    for o in (centre + np.array([0.0, 1.0, 6.0]), points[0] if hit.any() else centre):
        for k in range(3):
            for sgn in (1.0, -1.0):
                for zero in (0.0, -0.0):
                    d = np.full(3, zero)
                    d[k] = sgn
                    axis.append(np.concatenate([o, d]))
    axis = np.array(axis)
    rays = np.concatenate([cam, surface, placed, axis])
    n = len(rays)
    i = np.arange(n)
    offsets = np.where(i % 4 == 0, 0, np.where(i % 4 == 1, i, np.where(i % 4 == 2, 12345, MAX_OFFSET)))
    scaled = rays.copy()
    scaled[:, 3:] *= (10.0 ** rng.uniform(-3.0, 3.0, n))[:, None]
    return {"rays": f64(rays), "offsets": i32(offsets), "scaled": f64(scaled),
            "families": {"camera": len(cam), "surface": len(surface), "placed": len(placed), "axis": len(axis)}}


def left_fold(values, m, init=None, squares=False):
    """bin b = the left fold, in order, of values [b m, (b + 1) m) (or of their squares) onto init[b] (None: zeros)"""
    v = f64(values).reshape(-1, m, 3)
    acc = np.zeros((v.shape[0], 3)) if init is None else f64(init).copy()
    for k in range(m):
        acc = acc + (v[:, k] * v[:, k] if squares else v[:, k])
    return acc
