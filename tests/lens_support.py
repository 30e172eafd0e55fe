"""Shared by the thin-lens tests: builds and loads the restatement tests/c/lens_oracle.c (envlight_oracle.c, texture_oracle.c and the
oracle's source included unchanged, plus the lens ray and the one path loop that takes its camera ray as an argument, written out in
C from include/ptx.h), compiles the product's own rule (csrc/pt_lens.h) for the host, and holds the scenes and samples the CPU and
GPU tests share.

Both libraries are compiled into build/ (out of git).  The restatement carries its own copy of the oracle's globals, so its math mode
is set here, to the shared pt_math.h functions (0), before anything is compared with the GPU.
"""
import ctypes as C
import os
import re
import subprocess

import numpy as np

from path_tracer_ocaml_amd import abi
from texture_support import BILINEAR, REPEAT_U, REPEAT_V, ImageRecord, random_image, set_images  # noqa: F401

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
dp, ip = abi.c_double_p, abi.c_int32_p
_LIB = None
_PRODUCT = None
# tests/c/lens_oracle.c's ORCN_MUT_*
MUTANTS = {"focus measured along the ray": 1, "r = u for sqrt u": 2, "lens pair at dimensions 2 and 3": 3}


def _oracle_cflags():
    text = open(os.path.join(ROOT, "oracle", "Makefile")).read()
    return re.search(r"^CFLAGS\s*=\s*(.*)$", text, re.M).group(1).split()


def _build(so, deps, cmd):
    if not os.path.exists(so) or any(os.path.getmtime(d) > os.path.getmtime(so) for d in deps):
        os.makedirs(os.path.dirname(so), exist_ok=True)
        tmp = so + ".%d.tmp" % os.getpid()
        subprocess.check_call(cmd(tmp))
        os.replace(tmp, so)
    return so


def lib():
    global _LIB
    if _LIB is not None:
        return _LIB
    c = os.path.join(ROOT, "tests", "c")
    src = os.path.join(c, "lens_oracle.c")
    deps = [src, os.path.join(c, "envlight_oracle.c"), os.path.join(c, "texture_oracle.c"), os.path.join(ROOT, "oracle", "pt_oracle.c"),
            os.path.join(ROOT, "include", "ptx.h"), os.path.join(ROOT, "path_tracer_ocaml_amd", "csrc", "pt_math.h")]
    so = _build(os.path.join(ROOT, "build", "liblens_oracle.so"), deps,
                lambda tmp: [os.environ.get("CC", "gcc"), *_oracle_cflags(), "-shared", "-o", tmp, src, "-lm", "-lpthread"])
    L = C.CDLL(so)
    L.orc_set_math.argtypes = [C.c_int]
    L.orc_scene_create.restype = C.c_void_p
    L.orc_scene_create.argtypes = [C.POINTER(abi.SceneDesc)]
    L.orc_scene_destroy.argtypes = [C.c_void_p]
    L.orc_trace_samples.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int64, ip, ip, ip, dp, C.c_void_p]
    L.orcn_lens_rays.argtypes = [dp, C.c_double, C.c_double, C.c_int, C.c_int64, dp, dp, dp]
    L.orcn_sample_rays.argtypes = [C.c_void_p, C.c_double, C.c_double, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int64, ip, ip, ip,
                                   dp, dp]
    L.orcn_trace_samples.argtypes = [C.c_void_p, C.POINTER(ImageRecord), dp, C.c_int, C.c_int, C.c_int, dp, C.c_int, C.c_int, C.c_double,
                                     C.c_double, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int64, ip, ip, ip, dp,
                                     C.POINTER(C.c_int64)]
    L.orcn_first_hits.argtypes = [C.c_void_p, C.POINTER(ImageRecord), dp, C.c_int, C.c_int, C.c_int, dp, C.c_double, C.c_double, C.c_int,
                                  C.c_int, C.c_int, C.c_int, C.c_int64, ip, ip, ip, dp]
    L.orc_set_math(0)
    _LIB = L
    return L


_PRODUCT_SRC = """
#include "pt_lens.h"
extern "C" void product_lens_rays(const double* cam4, double A, double F, long long n, const double* cxcy, const double* uv, double* out) {
  for (long long i = 0; i < n; ++i) {
    V3 o, d;
    pt_lens_ray(cam4[0], cam4[1], cam4[2], cam4[3], cxcy[2 * i], cxcy[2 * i + 1], A, F, uv[2 * i], uv[2 * i + 1], &o, &d);
    out[6 * i] = o.x; out[6 * i + 1] = o.y; out[6 * i + 2] = o.z; out[6 * i + 3] = d.x; out[6 * i + 4] = d.y; out[6 * i + 5] = d.z;
  }
}
"""


def product():
    """csrc/pt_lens.h -- the function the kernels call -- compiled for the host with the library's floating-point flags"""
    global _PRODUCT
    if _PRODUCT is not None:
        return _PRODUCT
    csrc = os.path.join(ROOT, "path_tracer_ocaml_amd", "csrc")
    deps = [os.path.join(csrc, f) for f in ("pt_lens.h", "pt_vec.h", "pt_math.h")] + [os.path.abspath(__file__)]
    out_dir = os.path.join(ROOT, "build")
    os.makedirs(out_dir, exist_ok=True)
    src = os.path.join(out_dir, "lens_product.cpp")

    def cmd(tmp):
        with open(src, "w") as f:
            f.write(_PRODUCT_SRC)
        return [os.environ.get("CXX", "g++"), "-std=c++17", "-O2", "-fPIC", "-ffp-contract=off", "-fno-fast-math", "-march=x86-64-v3",
                "-I", csrc, "-shared", "-o", tmp, src]
    L = C.CDLL(_build(os.path.join(out_dir, "liblens_product.so"), deps, cmd))
    L.product_lens_rays.argtypes = [dp, C.c_double, C.c_double, C.c_longlong, dp, dp, dp]
    _PRODUCT = L
    return L


def _dp(a):
    return a.ctypes.data_as(dp)


def _ip(a):
    return a.ctypes.data_as(ip)


def f64(a):
    return np.ascontiguousarray(a, dtype=np.float64)


def i32(a):
    return np.ascontiguousarray(a, dtype=np.int32)


def bits(a):
    return f64(a).view(np.uint64)


def c_lens_rays(cam4, A, F, cxcy, uv, mutant=0):
    cam4, cxcy, uv = f64(cam4), f64(cxcy).reshape(-1, 2), f64(uv).reshape(-1, 2)
    out = np.zeros((len(uv), 6))
    lib().orcn_lens_rays(_dp(cam4), A, F, mutant, len(uv), _dp(cxcy), _dp(uv), _dp(out))
    return out


def product_lens_rays(cam4, A, F, cxcy, uv):
    cam4, cxcy, uv = f64(cam4), f64(cxcy).reshape(-1, 2), f64(uv).reshape(-1, 2)
    out = np.zeros((len(uv), 6))
    product().product_lens_rays(_dp(cam4), A, F, len(uv), _dp(cxcy), _dp(uv), _dp(out))
    return out


class Restatement:
    """A scene of the restatement library for a ptx_scene_desc pointer."""

    def __init__(self, desc_ptr, keepalive=None):
        self._keep = keepalive
        self._h = lib().orc_scene_create(desc_ptr)
        assert self._h
        self._n_textures = desc_ptr.contents.n_textures

    def _table(self, images):
        if not images:
            return None, None
        table = (ImageRecord * self._n_textures)()
        keep = []
        for index, (img, flags) in images.items():
            img = f64(img)
            keep.append(img)
            table[index].rgb, table[index].width, table[index].height, table[index].flags = _dp(img), img.shape[1], img.shape[0], flags
        return table, keep

    @staticmethod
    def _env(env):
        if env is None:
            return None, 0, 0, 0, None, None
        img, flags, R = env
        img, R = f64(img), f64(np.eye(3) if R is None else R).reshape(-1)
        return _dp(img), img.shape[1], img.shape[0], flags, _dp(R), (img, R)

    def oracle_samples(self, width, height, spp, max_bounces, xs, ys, passes):
        """orc_trace_samples: the oracle's own path loop"""
        xs, ys, passes = i32(xs), i32(ys), i32(passes)
        rgb = np.zeros((len(xs), 3))
        lib().orc_trace_samples(self._h, width, height, spp, max_bounces, len(xs), _ip(xs), _ip(ys), _ip(passes), _dp(rgb), None)
        return rgb

    def rays(self, lens, width, height, spp, max_bounces, xs, ys, passes, mutant=0):
        """(rays n x 6, film coordinates n x 2) of the samples' camera rays; lens = (A, F), A = 0: off"""
        xs, ys, passes = i32(xs), i32(ys), i32(passes)
        rays, cxcy = np.zeros((len(xs), 6)), np.zeros((len(xs), 2))
        lib().orcn_sample_rays(self._h, lens[0], lens[1], mutant, width, height, spp, max_bounces, len(xs), _ip(xs), _ip(ys), _ip(passes),
                               _dp(rays), _dp(cxcy))
        return rays, cxcy

    def trace_samples(self, lens, width, height, spp, max_bounces, xs, ys, passes, images=None, env=None, mode=0, sampling=False,
                      mutant=0):
        """(radiance n x 3, segments)"""
        xs, ys, passes = i32(xs), i32(ys), i32(passes)
        table, keep = self._table(images)
        e = self._env(env)
        rgb, seg = np.zeros((len(xs), 3)), C.c_int64(0)
        rc = lib().orcn_trace_samples(self._h, table, *e[:5], mode, int(sampling), lens[0], lens[1], mutant, width, height, spp,
                                      max_bounces, len(xs), _ip(xs), _ip(ys), _ip(passes), _dp(rgb), C.byref(seg))
        assert rc == 0, rc
        del keep
        return rgb, seg.value

    def first_hits(self, lens, width, height, spp, max_bounces, xs, ys, passes, images=None, env=None):
        """the feature records (n x 8) of the samples' camera rays"""
        xs, ys, passes = i32(xs), i32(ys), i32(passes)
        table, keep = self._table(images)
        e = self._env(env)
        feat = np.zeros((len(xs), 8))
        lib().orcn_first_hits(self._h, table, *e[:5], lens[0], lens[1], width, height, spp, max_bounces, len(xs), _ip(xs), _ip(ys),
                              _ip(passes), _dp(feat))
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
W, H, SPP = 13, 11, 3  # two tile columns and two tile rows, both ragged
DEPTHS = (0, 1, 4)
# name -> lighting modes.  shirley: Simd_leaf, LDS-resident (the scene that would otherwise take the shade-first order, the per-octant
# image and tile lists); mesh: walked from HBM / L2, its floor tested before the tree
CASES = {"shirley": (0,), "shirley_array": (0,), "cornell": (0, 1, 2), "mesh": (0,), "image": (0,), "envlight": (2,)}
_CACHE = {}


def all_samples(width=W, height=H, spp=SPP):
    """every (x, y, pass) of a frame, pixel-major: sample k of pixel j is entry j * spp + k"""
    ys, xs, ps = np.meshgrid(np.arange(height), np.arange(width), np.arange(spp), indexing="ij")
    return i32(xs.ravel()), i32(ys.ravel()), i32(ps.ravel())


def pass_order_sums(samples, width, height, spp):
    """the raw sums a render leaves: each pixel's samples added in pass order, from zero"""
    sums = np.zeros((height * width, 3))
    for p in range(spp):
        sums = sums + samples.reshape(height * width, spp, 3)[:, p]
    return sums.reshape(height, width, 3)


def case(name, oracle, width=W, height=H):
    """{"desc", "keep", "images", "env", "sampling", "lens": (A, F), "lds"}.  The lens is scaled to the scene: F is the median distance
    along -z of the pinhole's first hits (what the middle of the picture shows is in focus), A = F / 16 at first and doubled until the
    restatement's radiance at depth 4 differs from the pinhole's on some sample (test_lens_reference asserts both conditions)."""
    key = (name, width, height)
    if key in _CACHE:
        return _CACHE[key]
    images = env = None
    sampling, lds = False, None
    if name in ("shirley", "shirley_array", "image", "envlight"):
        desc = oracle.desc_shirley(width, height, no_simd=(name == "shirley_array"))
        ptr, keep = desc.ptr, desc
        lds = None if name == "shirley_array" else 1
        if name == "image":
            images = {0: (random_image(16, 8, 40), BILINEAR | REPEAT_U | REPEAT_V), 1: (random_image(2, 3, 41), BILINEAR | REPEAT_V),
                      2: (random_image(5, 3, 42), REPEAT_U)}
        if name == "envlight":
            import envlight_support as ES
            env, sampling = ES.environment(), True
    elif name == "cornell":
        desc = oracle.desc_cornell(width, height)
        ptr, keep, lds = desc.ptr, desc, 1
    elif name == "mesh":
        desc = oracle.desc_ganesha_like(width, height, n_target=6000)
        ptr, keep, lds = desc.ptr, desc, 0
    else:
        raise KeyError(name)
    ref = Restatement(ptr, keep)
    xs, ys, ps = all_samples(width, height, SPP)
    off = (0.0, 1.0)
    feat = ref.first_hits(off, width, height, SPP, 4, xs, ys, ps)
    rays, _ = ref.rays(off, width, height, SPP, 4, xs, ys, ps)
    hit = feat[:, 7] > 0
    assert hit.sum() >= len(xs) // 4, name
    focus = float(np.median((feat[:, 6] * -rays[:, 5])[hit]))
    mode = CASES[name][-1]
    pin, _ = ref.trace_samples(off, width, height, SPP, 4, xs, ys, ps, images, env, mode, sampling)
    radius = focus / 16.0
    for _ in range(8):
        got, _ = ref.trace_samples((radius, focus), width, height, SPP, 4, xs, ys, ps, images, env, mode, sampling)
        if (bits(got) != bits(pin)).any():
            break
        radius *= 2.0
    c = {"desc": ptr, "keep": keep, "images": images, "env": env, "sampling": sampling, "lens": (radius, focus), "lds": lds, "ref": ref}
    _CACHE[key] = c
    return c


def gpu_scene(P, c, mode=0, lens=True):
    """the GPU scene of a case: images, environment, sampling, lighting mode and (lens=True) its lens set"""
    g = P.Scene(c["desc"], 0, keepalive=c["keep"])
    if c["images"]:
        set_images(g, c["images"])
    if c["env"] is not None:
        img, flags, R = c["env"]
        g.set_environment(img, R, bilinear=bool(flags & BILINEAR))
    if c["sampling"]:
        g.set_environment_sampling(True)
    g.set_lighting(mode)
    if lens:
        g.set_lens(*c["lens"])
    return g


def restated(c, depth, mode=0, lens=True, width=W, height=H, spp=SPP, samples=None):
    """the restatement's (radiance, segments) for all samples of the frame (or `samples`), under the case's state"""
    xs, ys, ps = samples if samples is not None else all_samples(width, height, spp)
    return c["ref"].trace_samples(c["lens"] if lens else (0.0, 1.0), width, height, spp, depth, xs, ys, ps, c["images"], c["env"], mode,
                                  c["sampling"])
