"""Shared by the image-texture tests: builds and loads the restatement tests/c/texture_oracle.c (the oracle's source included
unchanged, plus the image rule and the environment written out in C from include/ptx.h), and the scenes the tests use.

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


def _oracle_cflags():
    text = open(os.path.join(ROOT, "oracle", "Makefile")).read()
    return re.search(r"^CFLAGS\s*=\s*(.*)$", text, re.M).group(1).split()


def lib():
    global _LIB
    if _LIB is not None:
        return _LIB
    src = os.path.join(ROOT, "tests", "c", "texture_oracle.c")
    deps = [src, os.path.join(ROOT, "oracle", "pt_oracle.c"), os.path.join(ROOT, "include", "ptx.h"),
            os.path.join(ROOT, "path_tracer_ocaml_amd", "csrc", "pt_math.h")]
    out_dir = os.path.join(ROOT, "build")
    so = os.path.join(out_dir, "libtexture_oracle.so")
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
    L.orct_image_eval.argtypes = [dp, C.c_int, C.c_int, C.c_int, C.c_int64, dp, dp]
    L.orct_environment_eval.argtypes = [dp, C.c_int, C.c_int, C.c_int, dp, C.c_int64, dp, dp]
    L.orct_trace_samples.argtypes = [C.c_void_p, dp, C.c_int, C.c_int, C.c_int, dp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int64,
                                     ip, ip, ip, dp]
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


def c_image_eval(img, flags, u, v):
    img = f64(img)
    uv = f64(np.stack([u, v], axis=1))
    out = np.zeros((len(uv), 3))
    lib().orct_image_eval(_dp(img), img.shape[1], img.shape[0], flags, len(uv), _dp(uv), _dp(out))
    return out


def c_environment_eval(img, flags, R, dirs):
    img, dirs = f64(img), f64(dirs)
    R = f64(np.eye(3) if R is None else R).reshape(-1)
    out = np.zeros((len(dirs), 3))
    lib().orct_environment_eval(_dp(img), img.shape[1], img.shape[0], flags, _dp(R), len(dirs), _dp(dirs), _dp(out))
    return out


class Restatement:
    """A scene of the restatement library for a ptx_scene_desc pointer, traced under an environment."""

    def __init__(self, desc_ptr, keepalive=None):
        self._keep = keepalive
        self._h = lib().orc_scene_create(desc_ptr)
        assert self._h

    def trace_samples(self, env, flags, R, width, height, spp, max_bounces, xs, ys, passes):
        env, xs, ys, passes = f64(env), i32(xs), i32(ys), i32(passes)
        R = f64(np.eye(3) if R is None else R).reshape(-1)
        rgb = np.zeros((len(xs), 3))
        lib().orct_trace_samples(self._h, _dp(env), env.shape[1], env.shape[0], flags, _dp(R), width, height, spp, max_bounces,
                                 len(xs), _ip(xs), _ip(ys), _ip(passes), _dp(rgb))
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


def all_samples(width, height, spp):
    """every (x, y, pass) of a frame, pixel-major: sample k of pixel j is entry j * spp + k"""
    ys, xs, ps = np.meshgrid(np.arange(height), np.arange(width), np.arange(spp), indexing="ij")
    return i32(xs.ravel()), i32(ys.ravel()), i32(ps.ravel())


def with_checker(src, index, width, height, even=(0.2, 0.3, 0.1), odd=(0.9, 0.9, 0.9)):
    """The oracle's scene descriptor `src` (an oracle.Desc) with entry `index` of its texture table replaced by
    Texture.checker ~width ~height (the cell counts are width - 1, height - 1): a copy of the descriptor and of the table, the
    arrays shared.  An entry that was a checker keeps its colours.  Returns (desc, keepalive)."""
    sd = src.d
    texs = (abi.Texture * sd.n_textures)()
    for i in range(sd.n_textures):
        C.memmove(C.byref(texs[i]), C.byref(sd.textures[i]), C.sizeof(abi.Texture))
    t = texs[index]
    if t.kind != abi.PTX_TEX_CHECKER:
        t.even[:] = list(even)
        t.odd[:] = list(odd)
    t.kind, t.width, t.height = abi.PTX_TEX_CHECKER, width, height
    d = abi.SceneDesc()
    C.memmove(C.byref(d), C.byref(sd), C.sizeof(abi.SceneDesc))
    d.textures = texs
    return d, (texs, src)


def checker_colours(desc, index):
    t = desc.textures[index]
    return np.array(list(t.even)), np.array(list(t.odd))


def random_environment(width, height, seed):
    """a finite HDR-like image with structure in both axes, so that a wrong row, column, wrap or weight shows"""
    rng = np.random.default_rng(seed)
    img = rng.uniform(0.0, 2.0, (height, width, 3))
    img[rng.integers(0, height), rng.integers(0, width)] = [40.0, 35.0, 30.0]  # a "sun"
    return img


def rotation(axis, degrees):
    """a proper rotation that is no permutation of the axes"""
    a = np.asarray(axis, dtype=np.float64)
    a = a / np.linalg.norm(a)
    t = np.deg2rad(degrees)
    K = np.array([[0.0, -a[2], a[1]], [a[2], 0.0, -a[0]], [-a[1], a[0], 0.0]])
    return np.eye(3) + np.sin(t) * K + (1.0 - np.cos(t)) * (K @ K)


def camera_rays(oracle, desc, width, height, spp, max_bounces, xs, ys, passes):
    """the camera ray of every listed sample, as sample_pixel makes it (integrator.ml:96-109): the oracle's sampler and Camera.ray"""
    xs, ys, passes = np.asarray(xs, dtype=np.int64), np.asarray(ys, dtype=np.int64), np.asarray(passes, dtype=np.int64)
    offsets = ys * width + xs + passes * spp
    n_dim = 2 + 2 * max_bounces
    dx = oracle.lds_get_vec(n_dim, offsets, np.zeros(len(xs), dtype=np.int64))
    dy = oracle.lds_get_vec(n_dim, offsets, np.ones(len(xs), dtype=np.int64))
    cx = (xs.astype(np.float64) + dx) * (1.0 / float(width))
    cy = 1.0 - ((ys.astype(np.float64) + dy) * (1.0 / float(height)))
    cam = f64([desc.camera.lower_left_x, desc.camera.lower_left_y, desc.camera.view_x, desc.camera.view_y])
    od = np.zeros((len(xs), 6))
    row = np.zeros(6)
    L = oracle.lib()
    for i in range(len(xs)):
        L.orc_camera_ray(_dp(cam), float(cx[i]), float(cy[i]), _dp(row))
        od[i] = row
    return od[:, :3], od[:, 3:]
