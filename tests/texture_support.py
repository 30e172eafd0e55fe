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
BILINEAR, REPEAT_U, REPEAT_V = 1, 2, 4
# tests/c/texture_oracle.c's ORCT_MUT_*: the rule restated wrongly in one way (the CPU tests' sensitivity conditions)
MUTANTS = {"u and v exchanged": 1, "v -> 1 - v": 2, "nearest for bilinear": 3, "ix + 1 for ix": 4, "row stride H for W": 5,
           "repeat in u toggled": 6, "repeat in v toggled": 7, "metal: the plain colour": 8}


class ImageRecord(C.Structure):
    """orct_image_t: one per texture-table index, width 0 = the descriptor's texture"""
    _fields_ = [("rgb", dp), ("width", C.c_int32), ("height", C.c_int32), ("flags", C.c_int32), ("reserved", C.c_int32)]


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
    L.orct_trace_samples_images.argtypes = [C.c_void_p, C.POINTER(ImageRecord), C.c_int, dp, C.c_int, C.c_int, C.c_int, dp, C.c_int,
                                            C.c_int, C.c_int, C.c_int, C.c_int64, ip, ip, ip, dp]
    L.orct_first_hits.argtypes = [C.c_void_p, C.POINTER(ImageRecord), C.c_int, dp, C.c_int, C.c_int, C.c_int, dp, C.c_int, C.c_int,
                                  C.c_int, C.c_int, C.c_int64, ip, ip, ip, dp, ip, ip, dp]
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
        self._n_textures = desc_ptr.contents.n_textures

    def trace_samples(self, env, flags, R, width, height, spp, max_bounces, xs, ys, passes):
        env, xs, ys, passes = f64(env), i32(xs), i32(ys), i32(passes)
        R = f64(np.eye(3) if R is None else R).reshape(-1)
        rgb = np.zeros((len(xs), 3))
        lib().orct_trace_samples(self._h, _dp(env), env.shape[1], env.shape[0], flags, _dp(R), width, height, spp, max_bounces,
                                 len(xs), _ip(xs), _ip(ys), _ip(passes), _dp(rgb))
        return rgb

    def _table(self, images):
        """images: {texture index: (img (H, W, 3), flags)} or None -> (orct_image_t array or None, keepalive)"""
        if not images:
            return None, None
        table = (ImageRecord * self._n_textures)()
        keep = []
        for index, (img, flags) in images.items():
            assert 0 <= index < self._n_textures
            img = f64(img)
            keep.append(img)
            table[index].rgb, table[index].width, table[index].height, table[index].flags = _dp(img), img.shape[1], img.shape[0], flags
        return table, keep

    @staticmethod
    def _env(env, env_flags, R):
        if env is None:
            return None, 0, 0, 0, None, None
        env = f64(env)
        R = f64(np.eye(3) if R is None else R).reshape(-1)
        return _dp(env), env.shape[1], env.shape[0], env_flags, _dp(R), (env, R)

    def trace_samples_images(self, images, width, height, spp, max_bounces, xs, ys, passes, env=None, env_flags=BILINEAR, R=None,
                             mutant=0):
        """per-sample radiance under an image table {texture index: (img, flags)} (or None) and an environment (or None)"""
        xs, ys, passes = i32(xs), i32(ys), i32(passes)
        table, keep = self._table(images)
        *e, keep_env = self._env(env, env_flags, R)
        rgb = np.zeros((len(xs), 3))
        lib().orct_trace_samples_images(self._h, table, mutant, *e, width, height, spp, max_bounces, len(xs), _ip(xs), _ip(ys),
                                        _ip(passes), _dp(rgb))
        del keep, keep_env
        return rgb

    def first_hits(self, images, width, height, spp, max_bounces, xs, ys, passes, env=None, env_flags=BILINEAR, R=None, mutant=0):
        """the first hit of every sample's camera ray: (albedo (n, 3), hit flag, texture index hit or -1, the hit's (u, v))"""
        xs, ys, passes = i32(xs), i32(ys), i32(passes)
        table, keep = self._table(images)
        *e, keep_env = self._env(env, env_flags, R)
        n = len(xs)
        albedo, hit, tex, uv = np.zeros((n, 3)), np.zeros(n, dtype=np.int32), np.zeros(n, dtype=np.int32), np.zeros((n, 2))
        lib().orct_first_hits(self._h, table, mutant, *e, width, height, spp, max_bounces, n, _ip(xs), _ip(ys), _ip(passes),
                              _dp(albedo), _ip(hit), _ip(tex), _dp(uv))
        del keep, keep_env
        return albedo, hit, tex, uv

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


class DerivedDesc:
    """a descriptor copied from an oracle.Desc and changed: .ptr and .d as oracle.Desc has them, the arrays it shares kept alive"""

    def __init__(self, d, *keep):
        self.d, self.ptr, self._keep = d, C.pointer(d), keep


def with_metal_triangles(src, every=2):
    """The oracle's scene descriptor `src` with every `every`-th mesh triangle moved to a new material: a Metal on the texture entry
    the triangle's material names.  A copy of the descriptor, of the material table and of tri_material; the rest is shared."""
    sd = src.d
    mats = (abi.Material * (sd.n_materials + 1))()
    C.memmove(mats, sd.materials, C.sizeof(abi.Material) * sd.n_materials)
    tri = (C.c_int32 * sd.n_triangles)()
    C.memmove(tri, sd.tri_material, 4 * sd.n_triangles)
    first = tri[0]
    assert all(tri[i] == first for i in range(sd.n_triangles)) and mats[first].kind == abi.PTX_MAT_LAMBERTIAN
    C.memmove(C.byref(mats[sd.n_materials]), C.byref(mats[first]), C.sizeof(abi.Material))
    mats[sd.n_materials].kind = abi.PTX_MAT_METAL
    for i in range(0, sd.n_triangles, every):
        tri[i] = sd.n_materials
    d = abi.SceneDesc()
    C.memmove(C.byref(d), C.byref(sd), C.sizeof(abi.SceneDesc))
    d.materials, d.n_materials, d.tri_material = mats, sd.n_materials + 1, tri
    return DerivedDesc(d, mats, tri, src)


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


# ------------------------------------------------------------------------------------ whole paths under non-periodic images
PATH_W, PATH_H, PATH_SPP, PATH_DEPTH = 64, 32, 4, 8
_CASES = {}


def random_image(width, height, seed):
    """seeded uniform texels with one bright one: no period, no symmetry, W != H at every use, so a shifted, flipped, transposed or
    mis-strided lookup shows"""
    rng = np.random.default_rng(seed)
    img = rng.uniform(0.05, 0.95, (height, width, 3))
    img[rng.integers(0, height), rng.integers(0, width)] = [3.0, 2.5, 2.0]
    return img


def first_hit_counts(desc, width=PATH_W, height=PATH_H, spp=PATH_SPP):
    """{texture index: the number of the frame's samples whose first hit evaluates it} (a dielectric evaluates none)"""
    xs, ys, ps = all_samples(width, height, spp)
    ref = Restatement(desc.ptr, desc)
    _, _, tex, _ = ref.first_hits(None, width, height, spp, PATH_DEPTH, xs, ys, ps)
    ref.close()
    return {int(k): int(n) for k, n in zip(*np.unique(tex[tex >= 0], return_counts=True))}


def small_sphere_entries(desc):
    """(texture entry of a small metal sphere, of a small Lambertian one) of Shirley's scene: of each kind the entry that is the
    first hit of the most samples of the frame (the lowest index among equals)"""
    a = desc.arrays()
    counts = first_hit_counts(desc)
    best = {}
    for r, m in zip(a["sphere_r"], a["sphere_material"]):
        kind, tex = int(a["materials"][m][0]), int(a["materials"][m][1])
        if r < 1.0 and kind in (abi.PTX_MAT_METAL, abi.PTX_MAT_LAMBERTIAN):
            key = (-counts.get(tex, 0), tex)
            if kind not in best or key < best[kind]:
                best[kind] = key
    return best[abi.PTX_MAT_METAL][1], best[abi.PTX_MAT_LAMBERTIAN][1]


def path_case(name, oracle):
    """The scenes and image sets the whole-path tests share, CPU and GPU: {"desc", "images": {texture index: (img, flags)},
    "env": (img, flags, R) (used by the cases that run under an environment), "swap": two imaged entries whose exchange is the
    "wrong texture index" mutation, "lds": tree in LDS (None: not asserted)}.  Built once per name."""
    if name in _CASES:
        return _CASES[name]
    B, RU, RV = BILINEAR, REPEAT_U, REPEAT_V
    w, h = PATH_W, PATH_H
    env = (random_environment(16, 8, 31), B, rotation([0.3, 1.0, 0.2], 50.0))
    if name in ("shirley", "shirley_array"):
        desc = oracle.desc_shirley(w, h, no_simd=(name == "shirley_array"))
        metal, lambertian = small_sphere_entries(desc)
        a = desc.arrays()
        assert [int(a["materials"][m][0]) for m in (0, 2, 3)] == [abi.PTX_MAT_LAMBERTIAN, abi.PTX_MAT_METAL, abi.PTX_MAT_LAMBERTIAN]
        assert [int(a["materials"][m][1]) for m in (0, 2, 3)] == [0, 1, 2] and list(a["sphere_r"][:4]) == [1000.0, 1.0, 1.0, 1.0]
        images = {0: (random_image(512, 1024, 40), B | RU | RV),  # the ground sphere of radius 1000
                  1: (random_image(2, 3, 41), B | RV),             # the big metal sphere
                  2: (random_image(5, 3, 42), RU),                 # the big Lambertian sphere
                  metal: (random_image(3, 2, 43), B | RU),         # a small metal sphere
                  lambertian: (random_image(1, 4, 44), 0)}         # a small Lambertian sphere
        case = {"desc": desc, "images": images, "env": env, "swap": (1, 2), "lds": 1 if name == "shirley" else None}
    elif name == "cornell":
        desc = oracle.desc_cornell(w, h)
        a = desc.arrays()
        kinds = {int(t): int(k) for k, t in a["materials"][:, :2] if int(k) != abi.PTX_MAT_DIELECTRIC}
        assert kinds[0] == kinds[6] == abi.PTX_MAT_METAL and kinds[3] == kinds[4] == kinds[5] == abi.PTX_MAT_LAMBERTIAN
        assert a["materials"][5][3:6].tolist() == [12.0, 12.0, 12.0] and int(a["materials"][5][1]) == 5  # the emitting ceiling
        images = {0: (random_image(3, 3, 50), B),            # the metal enclosure quads
                  4: (random_image(7, 5, 51), B | RV),       # the floor
                  5: (random_image(4, 6, 52), 0),            # the emitting ceiling
                  6: (random_image(2, 2, 53), B | RU | RV),  # the metal sphere
                  3: (random_image(6, 9, 54), 0)}            # a solid wall
        case = {"desc": desc, "images": images, "env": env, "swap": (4, 3), "lds": 1}
    elif name == "mesh":
        # every other mesh triangle a metal on the same entry: without one the scene cannot tell the metal formula from the colour
        desc = with_metal_triangles(oracle.desc_ganesha_like(w, h, n_target=6000))
        images = {0: (random_image(9, 4, 60), B),            # the mesh triangles, uv t00, t01, t11, Lambertian and metal
                  1: (random_image(64, 48, 61), RU | RV)}    # the two floor triangles
        case = {"desc": desc, "images": images, "env": env, "swap": (0, 1), "lds": 0}
    else:
        raise KeyError(name)
    _CASES[name] = case
    return case


def equivalence_case(name, oracle, w=PATH_W, h=PATH_H):
    """(descriptor with the even checker, keepalive, texture index, cells (W, H), frame width, height)"""
    if name == "shirley":
        return (*with_checker(oracle.desc_shirley(w, h), 0, 11, 21), 0, (10, 20), w, h)
    if name == "cornell":
        return (*with_checker(oracle.desc_cornell(w, h), 4, 11, 11), 4, (10, 10), w, h)
    return (*with_checker(oracle.desc_ganesha_like(w, h, n_target=6000), 1, 21, 11), 1, (20, 10), w, h)


def swapped(images, i, j):
    out = dict(images)
    out[i], out[j] = images[j], images[i]
    return out


def set_images(scene, images):
    """every image of a table on a GPU scene"""
    for index, (img, flags) in images.items():
        scene.set_texture_image(index, img, bilinear=bool(flags & BILINEAR), repeat=(bool(flags & REPEAT_U), bool(flags & REPEAT_V)))


def pass_order_sums(samples, width, height, spp):
    """the raw sums a render leaves: each pixel's samples added in pass order, from zero"""
    sums = np.zeros((height * width, 3))
    for p in range(spp):
        sums = sums + samples.reshape(height * width, spp, 3)[:, p]
    return sums.reshape(height, width, 3)
