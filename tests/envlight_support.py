"""Shared by the environment-sampling tests: builds and loads the restatement tests/c/envlight_oracle.c (texture_oracle.c and, through
it, the oracle's source included unchanged, plus the density, the two sampling functions and the mixture written out in C from
include/ptx.h), and the images, scenes and samples the tests use.

The library is compiled with oracle/Makefile's flags into build/ (out of git).  It carries its own copy of the oracle's globals, so
its math mode is set here, to the shared pt_math.h functions (0), before anything is compared with the GPU.
"""
import ctypes as C
import os
import re
import subprocess

import numpy as np

from path_tracer_ocaml_amd import abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
dp, ip = abi.c_double_p, abi.c_int32_p
_LIB = None
BILINEAR = 1
MUTANTS = {"pd without 1 / sin(theta)": 1, "weights 0.5 / 0.5 for 0.25 / 0.25": 2}


def _oracle_cflags():
    text = open(os.path.join(ROOT, "oracle", "Makefile")).read()
    return re.search(r"^CFLAGS\s*=\s*(.*)$", text, re.M).group(1).split()


def lib():
    global _LIB
    if _LIB is not None:
        return _LIB
    src = os.path.join(ROOT, "tests", "c", "envlight_oracle.c")
    deps = [src, os.path.join(ROOT, "tests", "c", "texture_oracle.c"), os.path.join(ROOT, "oracle", "pt_oracle.c"),
            os.path.join(ROOT, "include", "ptx.h"), os.path.join(ROOT, "path_tracer_ocaml_amd", "csrc", "pt_math.h")]
    out_dir = os.path.join(ROOT, "build")
    so = os.path.join(out_dir, "libenvlight_oracle.so")
    if not os.path.exists(so) or any(os.path.getmtime(d) > os.path.getmtime(so) for d in deps):
        os.makedirs(out_dir, exist_ok=True)
        tmp = so + ".%d.tmp" % os.getpid()
        subprocess.check_call([os.environ.get("CC", "gcc"), *_oracle_cflags(), "-shared", "-o", tmp, src, "-lm", "-lpthread"])
        os.replace(tmp, so)
    L = C.CDLL(so)
    L.orc_set_math.argtypes = [C.c_int]
    L.orc_scene_create.restype = C.c_void_p
    L.orc_scene_create.argtypes = [C.POINTER(abi.SceneDesc)]
    L.orc_scene_destroy.argtypes = [C.c_void_p]
    L.orce_distribution.restype = C.c_double
    L.orce_distribution.argtypes = [dp, C.c_int, C.c_int, dp, dp]
    L.orce_sample_many.argtypes = [dp, C.c_int, C.c_int, dp, C.c_int64, dp, dp, ip]
    L.orce_pd_many.argtypes = [dp, C.c_int, C.c_int, dp, C.c_int64, dp, dp, ip]
    L.orce_trace_samples.argtypes = [C.c_void_p, dp, C.c_int, C.c_int, C.c_int, dp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                     C.c_int, C.c_int, C.c_int64, ip, ip, ip, dp]
    L.orc_set_math(0)
    _LIB = L
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


def _rot(R):
    return f64(np.eye(3) if R is None else R).reshape(-1)


def c_distribution(img):
    img = f64(img)
    H, W = img.shape[:2]
    m, c = np.zeros(H), np.zeros((H, W))
    T = lib().orce_distribution(_dp(img), W, H, _dp(m), _dp(c))
    return m, c, T


def c_sample(img, R, ab):
    img, ab, R = f64(img), f64(ab).reshape(-1, 2), _rot(R)
    dirs, texel = np.zeros((len(ab), 3)), np.zeros((len(ab), 2), dtype=np.int32)
    lib().orce_sample_many(_dp(img), img.shape[1], img.shape[0], _dp(R), len(ab), _dp(ab), _dp(dirs), _ip(texel))
    return dirs, texel


def c_pd(img, R, dirs):
    img, dirs, R = f64(img), f64(dirs).reshape(-1, 3), _rot(R)
    out, texel = np.zeros(len(dirs)), np.zeros((len(dirs), 2), dtype=np.int32)
    lib().orce_pd_many(_dp(img), img.shape[1], img.shape[0], _dp(R), len(dirs), _dp(dirs), _dp(out), _ip(texel))
    return out, texel


class Restatement:
    """A scene of the restatement library for a ptx_scene_desc pointer, traced under an environment in lighting mode 1 or 2."""

    def __init__(self, desc_ptr, keepalive=None):
        self._keep = keepalive
        self._h = lib().orc_scene_create(desc_ptr)
        assert self._h

    def trace_samples(self, env, flags, R, mode, sampling, width, height, spp, max_bounces, xs, ys, passes, mutant=0):
        env, xs, ys, passes, R = f64(env), i32(xs), i32(ys), i32(passes), _rot(R)
        rgb = np.zeros((len(xs), 3))
        rc = lib().orce_trace_samples(self._h, _dp(env), env.shape[1], env.shape[0], flags, _dp(R), mode, int(sampling), mutant, width,
                                      height, spp, max_bounces, len(xs), _ip(xs), _ip(ys), _ip(passes), _dp(rgb))
        assert rc == 0, rc
        return rgb

    def close(self):
        if self._h:
            lib().orc_scene_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


# ------------------------------------------------------------------------------------------------ images
def random_image(width, height, seed):
    rng = np.random.default_rng(seed)
    return rng.uniform(0.0, 2.0, (height, width, 3))


def sun_sky(width=64, height=32, sun=(40, 22), sun_rgb=(6000.0, 5500.0, 5000.0), seed=5):
    """a dim sky without period or symmetry and one bright texel ("the sun") in the upper half (row 0 is straight down)"""
    rng = np.random.default_rng(seed)
    img = rng.uniform(0.05, 0.15, (height, width, 3))
    img[sun[1], sun[0]] = sun_rgb
    return img


def table_images():
    """the images of the issue's density-table list: name -> (H, W, 3)"""
    out = {f"random {w}x{h}": random_image(w, h, 100 + w * 31 + h) for w, h in ((16, 8), (5, 3), (1, 1), (1, 7), (9, 1))}
    z = random_image(7, 6, 7)
    z[2, :] = 0.0
    z[:, 3] = 0.0
    z[5, :] = 0.0  # the last row too: the row fallback is not the last row
    z[:, 6] = 0.0  # the last column too
    out["zero rows and columns"] = z
    one = np.zeros((5, 6, 3))
    one[3, 2] = [0.5, 0.25, 2.0]
    out["one non-zero texel"] = one
    neg = random_image(6, 4, 9) - 0.9
    out["negative texels"] = neg
    return out


def rotation(axis, degrees):
    import texture_support
    return texture_support.rotation(axis, degrees)


def edge_pairs():
    e = [0.0, 0.25, 0.5, 1.0 - 2.0 ** -53]
    return np.array([(a, b) for a in e for b in e])


def edge_directions():
    d = [(0, 1, 0), (0, -1, 0), (1, 0, 0), (-1, 0, 0), (0, 0, 1), (0, 0, -1), (1, 1, 0), (0, 1, 1), (1, 0, 1), (-1, 0, 1e-300),
         (0.0, 2.0, 0.0), (1e-200, 1.0, 0.0), (-1.0, 0.0, -0.0), (-1.0, 0.0, 0.0), (3.0, -4.0, 0.0)]
    return np.array(d, dtype=np.float64)


def uniform_directions(n, seed):
    rng = np.random.default_rng(seed)
    z = rng.uniform(-1.0, 1.0, n)
    phi = rng.uniform(0.0, 2.0 * np.pi, n)
    s = np.sqrt(1.0 - z * z)
    return np.stack([s * np.cos(phi), z, s * np.sin(phi)], axis=1)


# ------------------------------------------------------------------------------------------------ scenes for whole paths
W, H, SPP, N = 96, 48, 16, 20000
DEPTHS = (1, 2, 8)
SCENES = ("shirley", "shirley_array", "open_lamp", "mesh_lamp")
ENV = {"env": None}


def environment():
    """(image, flags, R) every whole-path case runs under: the 64 x 32 sun sky, bilinear, under a rotation"""
    if ENV["env"] is None:
        ENV["env"] = (sun_sky(), BILINEAR, rotation([0.3, 1.0, 0.2], 50.0))
    return ENV["env"]


def descs(name, w=W, h=H):
    """(ptx_scene_desc pointer, keepalive, has light triangles, expected traversal_in_lds)"""
    from oracle import oracle as O
    import lighting_support as LS
    if name in ("shirley", "shirley_array"):
        d = O.desc_shirley(w, h, no_simd=(name == "shirley_array"))
        return d.ptr, d, False, (1 if name == "shirley" else None)
    if name == "open_lamp":  # a small mesh on its floor under a two-triangle lamp, open to the sky
        d, keep = LS.mesh_with_lamp(O, w, h, n_target=150)
        return C.pointer(d), (d, keep), True, 1
    d, keep = LS.mesh_with_lamp(O, w, h)  # >= 4000 triangles: walked from HBM / L2
    return C.pointer(d), (d, keep), True, 0


def samples(n=N, w=W, h=H, spp=SPP, seed=11):
    rng = np.random.default_rng(seed)
    return rng.integers(0, w, n), rng.integers(0, h, n), rng.integers(0, spp, n)


def all_samples(width, height, spp):
    ys, xs, ps = np.meshgrid(np.arange(height), np.arange(width), np.arange(spp), indexing="ij")
    return i32(xs.ravel()), i32(ys.ravel()), i32(ps.ravel())


def gpu_scene(P, name, sampling=True, mode=2, w=W, h=H):
    """the GPU scene of `name` under environment(), sampling and lighting mode set"""
    ptr, keep, _, _ = descs(name, w, h)
    g = P.Scene(ptr, 0, keepalive=keep)
    img, flags, R = environment()
    g.set_environment(img, R, bilinear=bool(flags & BILINEAR))
    if sampling:
        g.set_environment_sampling(True)
    g.set_lighting(mode)
    return g
