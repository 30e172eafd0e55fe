"""Shared by the sphere-light tests: builds and loads the restatement tests/c/spherelight_oracle.c (envlight_oracle.c, texture_oracle.c and,
through them, the oracle's source included unchanged, plus the joined light table, the cone rule and the mixture written out in C from
include/ptx.h), and the scenes and samples the tests use.

The library is compiled with oracle/Makefile's flags into build/ (out of git).  It carries its own copy of the oracle's globals, so
its math mode is set here, to the shared pt_math.h functions (0), before anything is compared with the GPU.
"""
import ctypes as C
import os
import subprocess

import numpy as np

from path_tracer_ocaml_amd import abi
import envlight_support as ES

ROOT = ES.ROOT
dp, ip = abi.c_double_p, abi.c_int32_p
_dp, _ip, f64, i32, bits = ES._dp, ES._ip, ES.f64, ES.i32, ES.bits
_LIB = None
MAX_SPHERES = 64
MUTANTS = {"pd without W_k / W_total": 1, "4 pi used for 2 pi q": 2}


def lib():
    global _LIB
    if _LIB is not None:
        return _LIB
    src = os.path.join(ROOT, "tests", "c", "spherelight_oracle.c")
    deps = [src, os.path.join(ROOT, "tests", "c", "envlight_oracle.c"), os.path.join(ROOT, "tests", "c", "texture_oracle.c"),
            os.path.join(ROOT, "oracle", "pt_oracle.c"), os.path.join(ROOT, "include", "ptx.h"),
            os.path.join(ROOT, "path_tracer_ocaml_amd", "csrc", "pt_math.h")]
    out_dir = os.path.join(ROOT, "build")
    so = os.path.join(out_dir, "libspherelight_oracle.so")
    if not os.path.exists(so) or any(os.path.getmtime(d) > os.path.getmtime(so) for d in deps):
        os.makedirs(out_dir, exist_ok=True)
        tmp = so + ".%d.tmp" % os.getpid()
        subprocess.check_call([os.environ.get("CC", "gcc"), *ES._oracle_cflags(), "-shared", "-o", tmp, src, "-lm", "-lpthread"])
        os.replace(tmp, so)
    L = C.CDLL(so)
    L.orc_set_math.argtypes = [C.c_int]
    L.orc_scene_create.restype = C.c_void_p
    L.orc_scene_create.argtypes = [C.POINTER(abi.SceneDesc)]
    L.orc_scene_destroy.argtypes = [C.c_void_p]
    L.orcs_table.restype = C.c_double
    L.orcs_table.argtypes = [C.c_void_p, ip, dp, dp]
    L.orcs_sample_many.argtypes = [C.c_void_p, C.c_int64, dp, dp, dp, ip]
    L.orcs_pd_many.argtypes = [C.c_void_p, C.c_int, C.c_int64, dp, dp, dp]
    L.orcs_trace_samples.argtypes = [C.c_void_p, dp, C.c_int, C.c_int, C.c_int, dp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                     C.c_int, C.c_int, C.c_int64, ip, ip, ip, dp]
    L.orc_set_math(0)
    _LIB = L
    return L


class Restatement:
    """A scene of the restatement library for a ptx_scene_desc pointer."""

    def __init__(self, desc_ptr, keepalive=None):
        self._keep = keepalive
        self._h = lib().orc_scene_create(desc_ptr)
        assert self._h

    def table(self):
        """(light triangles found, emissive spheres found, triangle records (n, 14), sphere records (n, 8), W_total)"""
        counts = np.zeros(2, dtype=np.int32)
        tri, sph = np.zeros((abi.PTX_MAX_LIGHT_TRIANGLES, 14)), np.zeros((MAX_SPHERES, 8))
        total = lib().orcs_table(self._h, _ip(counts), _dp(tri), _dp(sph))
        nt = int(counts[0]) if counts[0] <= abi.PTX_MAX_LIGHT_TRIANGLES else 0
        ns = int(counts[1]) if counts[1] <= MAX_SPHERES else 0
        return int(counts[0]), int(counts[1]), tri[:nt].copy(), sph[:ns].copy(), total

    def sample(self, points, uv):
        p, uv = f64(points).reshape(-1, 3), f64(uv).reshape(-1, 2)
        dirs, index = np.zeros((len(p), 3)), np.zeros(len(p), dtype=np.int32)
        assert lib().orcs_sample_many(self._h, len(p), _dp(p), _dp(uv), _dp(dirs), _ip(index)) == 0
        return dirs, index

    def pd(self, points, dirs, mutant=0):
        p, d = f64(points).reshape(-1, 3), f64(dirs).reshape(-1, 3)
        out = np.zeros(len(p))
        assert lib().orcs_pd_many(self._h, mutant, len(p), _dp(p), _dp(d), _dp(out)) == 0
        return out

    def trace_samples(self, mode, spheres_on, width, height, spp, max_bounces, xs, ys, passes, env=None, env_sampling=False, mutant=0):
        """env: None or (image, flags, R)"""
        xs, ys, passes = i32(xs), i32(ys), i32(passes)
        rgb = np.zeros((len(xs), 3))
        img = f64(env[0]) if env is not None else None
        R = ES._rot(env[2]) if env is not None else None
        rc = lib().orcs_trace_samples(self._h, _dp(img) if env is not None else None, img.shape[1] if env is not None else 0,
                                      img.shape[0] if env is not None else 0, env[1] if env is not None else 0,
                                      _dp(R) if env is not None else None, mode, int(spheres_on), int(env_sampling), mutant, width, height,
                                      spp, max_bounces, len(xs), _ip(xs), _ip(ys), _ip(passes), _dp(rgb))
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


# ------------------------------------------------------------------------------------------------ scene descriptions
def with_spheres(src, spheres, leaf_kind=None):
    """The description `src` (an oracle Desc, or an (abi.SceneDesc, keepalive) pair) with spheres appended to its build list, each
    (x, y, z, r, emit, albedo) a Lambertian sphere of a solid texture `albedo` that emits `emit` in every channel (0: it does not).
    The spheres come AFTER the description's own.  Returns (abi.SceneDesc, keepalive)."""
    if isinstance(src, tuple):
        sd, src_keep = src
    else:
        sd, src_keep = src.d, src

    def arr(p, n, dt):
        return np.ctypeslib.as_array(p, shape=(n,)).copy() if n and p else np.zeros(0, dtype=dt)

    sp = np.asarray(spheres, dtype=np.float64).reshape(-1, 6)
    n0, k, nm, ntx = sd.n_spheres, len(sp), sd.n_materials, sd.n_textures
    keep = {
        "sx": np.concatenate([arr(sd.sphere_x, n0, np.float64), sp[:, 0]]), "sy": np.concatenate([arr(sd.sphere_y, n0, np.float64), sp[:, 1]]),
        "sz": np.concatenate([arr(sd.sphere_z, n0, np.float64), sp[:, 2]]), "sr": np.concatenate([arr(sd.sphere_r, n0, np.float64), sp[:, 3]]),
        "sm": np.concatenate([arr(sd.sphere_material, n0, np.int32), nm + np.arange(k, dtype=np.int32)]).astype(np.int32),
    }
    keep = {name: np.ascontiguousarray(v) for name, v in keep.items()}
    mats = (abi.Material * (nm + k))()
    for i in range(nm):
        C.memmove(C.byref(mats[i]), C.byref(sd.materials[i]), C.sizeof(abi.Material))
    texs = (abi.Texture * (ntx + k))()
    for i in range(ntx):
        C.memmove(C.byref(texs[i]), C.byref(sd.textures[i]), C.sizeof(abi.Texture))
    for i in range(k):
        texs[ntx + i].kind = abi.PTX_TEX_SOLID
        texs[ntx + i].even[:] = [sp[i, 5]] * 3
        mats[nm + i].kind, mats[nm + i].texture = abi.PTX_MAT_LAMBERTIAN, ntx + i
        mats[nm + i].emit[:] = [sp[i, 4]] * 3
    d = abi.SceneDesc()
    C.memmove(C.byref(d), C.byref(sd), C.sizeof(abi.SceneDesc))
    d.n_spheres = n0 + k
    d.sphere_x, d.sphere_y, d.sphere_z, d.sphere_r = _dp(keep["sx"]), _dp(keep["sy"]), _dp(keep["sz"]), _dp(keep["sr"])
    d.sphere_material = _ip(keep["sm"])
    d.n_materials, d.materials, d.n_textures, d.textures = nm + k, mats, ntx + k, texs
    if leaf_kind is not None:
        d.leaf_kind = leaf_kind
    return d, (keep, mats, texs, src_keep)


def plane_scene(lamps, albedo=0.7, depth=5.0):
    """A Lambertian plane z = -depth facing the camera (at the origin, looking down -z, black background) that fills the view, under the
    sphere lamps (x, y, z, r, emit), which lie outside the view.  Returns (abi.SceneDesc, keepalive)."""
    big = 1000.0
    keep = {
        "vx": np.array([-big, big, big, -big]), "vy": np.array([-big, -big, big, big]), "vz": np.full(4, -depth),
        "idx": np.array([0, 1, 2, 0, 2, 3], dtype=np.int32), "uv": np.array([0.0, 0, 1, 0, 1, 1, 0, 0, 1, 1, 0, 1]),
        "tm": np.zeros(2, dtype=np.int32),
    }
    mats, texs = (abi.Material * 1)(), (abi.Texture * 1)()
    texs[0].kind = abi.PTX_TEX_SOLID
    texs[0].even[:] = [albedo] * 3
    mats[0].kind, mats[0].texture = abi.PTX_MAT_LAMBERTIAN, 0
    d = abi.SceneDesc()
    d.n_vertices, d.n_triangles = 4, 2
    d.vertex_x, d.vertex_y, d.vertex_z = _dp(keep["vx"]), _dp(keep["vy"]), _dp(keep["vz"])
    d.tri_indices, d.tri_uv, d.tri_material = _ip(keep["idx"]), _dp(keep["uv"]), _ip(keep["tm"])
    d.n_materials, d.materials, d.n_textures, d.textures = 1, mats, 1, texs
    d.camera.lower_left_x, d.camera.lower_left_y, d.camera.view_x, d.camera.view_y = -1.0, -0.5, 2.0, 1.0
    d.background.kind = abi.PTX_BG_BLACK
    d.leaf_kind, d.length_cutoff, d.num_bins = abi.PTX_LEAF_ARRAY, 2, 32
    return with_spheres((d, (keep, mats, texs)), [(x, y, z, r, e, 1.0) for x, y, z, r, e in lamps])


def shirley_lamp_position(oracle, width, height):
    """a point three units above the middle of the Shirley scene's small spheres, along the ground sphere's normal there"""
    a = oracle.desc_shirley(width, height).arrays()
    c = np.stack([a["sphere_x"], a["sphere_y"], a["sphere_z"]], axis=1)
    g = int(a["sphere_r"].argmax())
    mid = np.delete(c, g, axis=0).mean(axis=0)
    up = (mid - c[g]) / np.linalg.norm(mid - c[g])
    return mid + 3.0 * up


W, H, SPP, N = 32, 16, 64, 20000
DEPTHS = (1, 2, 8)
SCENES = ("shirley", "shirley_array", "cornell", "mesh", "env3", "inside")
LAMP_R, LAMP_EMIT = 0.5, 40.0
_ENV = {}


def environment():
    """(image, flags, R) of the three-way mixture's scene"""
    if "env" not in _ENV:
        _ENV["env"] = (ES.sun_sky(), ES.BILINEAR, ES.rotation([0.3, 1.0, 0.2], 50.0))
    return _ENV["env"]


def descs(name, w=W, h=H, lamp_r=LAMP_R):
    """The Shirley scenes are lit by one lamp sphere above the small spheres, under a black background.
    (ptx_scene_desc pointer, keepalive, light triangles expected, expected traversal_in_lds or None, environment or None)"""
    from oracle import oracle as O
    import lighting_support as LS
    if name in ("shirley", "shirley_array", "env3"):
        p = shirley_lamp_position(O, w, h)
        d, keep = with_spheres(O.desc_shirley(w, h, no_simd=(name == "shirley_array")), [(*p, lamp_r, LAMP_EMIT, 1.0)])
        d.background.kind = abi.PTX_BG_BLACK  # night: the lamp alone lights the scene (env3: the environment takes the background's place)
        return C.pointer(d), (d, keep), False, (None if name == "shirley_array" else 1), (environment() if name == "env3" else None)
    if name == "inside":  # the camera, and every hit, inside one dim emissive sphere that encloses the scene
        d, keep = with_spheres(O.desc_shirley(w, h), [(0.0, 0.0, 0.0, 4000.0, 0.25, 0.5)])
        return C.pointer(d), (d, keep), False, 1, None
    if name == "cornell":  # the ceiling's two triangles and a small lamp sphere inside the box
        d, keep = with_spheres(O.desc_cornell(w, h), [(0.2, 0.22, -1.5, 0.06, LAMP_EMIT, 1.0)])
        return C.pointer(d), (d, keep), True, 1, None
    if name == "cornell_dark":  # spheres that do not emit
        d = O.desc_cornell(w, h)
        return d.ptr, d, True, 1, None
    assert name == "mesh"  # >= 4000 triangles: walked from HBM / L2; a lamp quad and a lamp sphere beside it
    src, src_keep = LS.mesh_with_lamp(O, w, h)
    vx, vy, vz = (np.ctypeslib.as_array(p, shape=(src.n_vertices,)) for p in (src.vertex_x, src.vertex_y, src.vertex_z))
    ext = vx[:-4].max() - vx[:-4].min()
    d, keep = with_spheres((src, src_keep), [(float(vx[-4:].mean() + ext / 3.0), float(vy[-1]), float(vz[-4:].mean()), float(ext / 20.0), 60.0, 1.0)])
    return C.pointer(d), (d, keep), True, 0, None


def samples(n=N, w=W, h=H, spp=SPP, seed=13):
    rng = np.random.default_rng(seed)
    return rng.integers(0, w, n), rng.integers(0, h, n), rng.integers(0, spp, n)


def gpu_scene(P, name, on=True, mode=2, w=W, h=H, device=0):
    ptr, keep, _, _, env = descs(name, w, h)
    g = P.Scene(ptr, device, keepalive=keep)
    if env is not None:
        g.set_environment(env[0], env[2], bilinear=bool(env[1] & ES.BILINEAR))
        g.set_environment_sampling(True)
    if on:
        g.set_sphere_light_sampling(True)
    g.set_lighting(mode)
    return g
