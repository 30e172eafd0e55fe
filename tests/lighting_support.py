"""Shared by the lighting tests: builds and loads the restatement tests/c/lighting_oracle.c (the oracle's source included
unchanged, plus the light list and the lighting rule of DESIGN.md section 7) and the scenes and statistics they use.

The library is compiled with oracle/Makefile's flags into build/ (out of git).  It carries its own copy of the oracle's
globals, so its math mode is set here, to the shared pt_math.h functions (0), before anything is compared with the GPU.
Scene descriptions are plain ptx_scene_desc pointers: one made by oracle.desc_cornell or by the host mirror works.
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

# the four emitters of the issue's table: (ceiling_emit, lamp) with lamp = (half side, y, emit) or None
SCENES = {
    "ceiling12": (12.0, None),
    "lamp012": (0.0, (0.12, 0.999, 100.0)),
    "lamp003": (0.0, (0.03, 0.999, 400.0)),
    "lamp004_enclosed": (0.0, (0.04, 0.82, 400.0)),
}


def _oracle_cflags():
    text = open(os.path.join(ROOT, "oracle", "Makefile")).read()
    return re.search(r"^CFLAGS\s*=\s*(.*)$", text, re.M).group(1).split()


def lib():
    global _LIB
    if _LIB is not None:
        return _LIB
    src = os.path.join(ROOT, "tests", "c", "lighting_oracle.c")
    deps = [src, os.path.join(ROOT, "oracle", "pt_oracle.c"), os.path.join(ROOT, "include", "ptx.h"),
            os.path.join(ROOT, "path_tracer_ocaml_amd", "csrc", "pt_math.h")]
    out_dir = os.path.join(ROOT, "build")
    so = os.path.join(out_dir, "liblighting_oracle.so")
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
    L.orc_trace_samples.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int64, ip, ip, ip, dp, C.POINTER(C.c_int64)]
    L.orcl_lights.argtypes = [C.c_void_p, dp, dp]
    L.orcl_light_pd.restype = C.c_double
    L.orcl_light_pd.argtypes = [C.c_void_p, dp, dp]
    L.orcl_light_pd_many.argtypes = [C.c_void_p, dp, C.c_int64, dp, dp]
    L.orcl_trace_samples.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int64, ip, ip, ip, dp]
    L.orc_set_math(0)
    _LIB = L
    return L


def _dp(a):
    return a.ctypes.data_as(dp)


def _ip(a):
    return a.ctypes.data_as(ip)


def i32(a):
    return np.ascontiguousarray(a, dtype=np.int32)


class Restatement:
    """A scene of the restatement library (its own orc_scene_create) for a ptx_scene_desc pointer."""

    def __init__(self, desc_ptr, keepalive=None):
        self._keep = keepalive
        self._h = lib().orc_scene_create(desc_ptr)
        assert self._h

    def lights(self):
        """(count, total area, table of 14 doubles per light: a, b, c, n, A, cum)"""
        area = C.c_double(0.0)
        table = np.zeros((abi.PTX_MAX_LIGHT_TRIANGLES, 14))
        n = lib().orcl_lights(self._h, C.byref(area), _dp(table))
        return n, area.value, table[:min(n, abi.PTX_MAX_LIGHT_TRIANGLES)]

    def light_pd(self, p, w):
        p, w = np.ascontiguousarray(p, dtype=np.float64), np.ascontiguousarray(w, dtype=np.float64)
        return lib().orcl_light_pd(self._h, _dp(p), _dp(w))

    def light_pd_many(self, p, ws):
        p = np.ascontiguousarray(p, dtype=np.float64)
        ws = np.ascontiguousarray(ws, dtype=np.float64)
        out = np.zeros(ws.shape[0])
        assert lib().orcl_light_pd_many(self._h, _dp(p), ws.shape[0], _dp(ws), _dp(out)) == 0
        return out

    def trace_samples(self, mode, width, height, spp, max_bounces, xs, ys, passes):
        xs, ys, passes = i32(xs), i32(ys), i32(passes)
        rgb = np.zeros((len(xs), 3))
        rc = lib().orcl_trace_samples(self._h, mode, width, height, spp, max_bounces, len(xs), _ip(xs), _ip(ys), _ip(passes), _dp(rgb))
        assert rc == 0, rc
        return rgb

    def trace_samples_oracle(self, width, height, spp, max_bounces, xs, ys, passes):
        """the included oracle's own orc_trace_samples"""
        xs, ys, passes = i32(xs), i32(ys), i32(passes)
        rgb = np.zeros((len(xs), 3))
        lib().orc_trace_samples(self._h, width, height, spp, max_bounces, len(xs), _ip(xs), _ip(ys), _ip(passes), _dp(rgb), None)
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


def host_scene(name, width, height):
    """One of SCENES through the host mirror (pth_scene_cornell / pth_scene_cornell_lamp)."""
    from path_tracer_ocaml_amd import host
    ceiling, lamp = SCENES[name]
    if lamp is None:
        return host.cornell_box(width, height, ceiling)
    return host.cornell_lamp(width, height, ceiling, *lamp)


def all_samples(width, height, spp):
    """every (x, y, pass) of a frame, pixel-major: sample k of pixel j is entry j * spp + k"""
    ys, xs, ps = np.meshgrid(np.arange(height), np.arange(width), np.arange(spp), indexing="ij")
    return i32(xs.ravel()), i32(ys.ravel()), i32(ps.ravel())


def frame_stats(rgb, npix, spp):
    """luminance (r + g + b) / 3 per sample -> (frame mean, its iid standard error, per-pixel sample variance)"""
    y = rgb.sum(axis=1) / 3.0
    mean = float(y.mean())
    se = float(y.std(ddof=1) / np.sqrt(y.size))
    var = y.reshape(npix, spp).var(axis=1, ddof=1)
    return mean, se, var


def mesh_with_lamp(oracle, width, height, n_target=6000, emit=60.0):
    """The synthetic mesh scene (walked from HBM / L2 at this size) with a two-triangle lamp appended to its build list: a square
    above the mesh, facing down, about a third of the mesh's extent across.  Returns (desc, keepalive)."""
    import ctypes
    src = oracle.desc_ganesha_like(width, height, n_target=n_target)
    a, sd = src.arrays(), src.d
    vx, vy, vz = a["vertex_x"], a["vertex_y"], a["vertex_z"]
    lo = np.array([vx.min(), vy.min(), vz.min()])
    hi = np.array([vx.max(), vy.max(), vz.max()])
    mid, ext = (lo + hi) / 2.0, (hi - lo)
    half, y = ext[0] / 6.0, hi[1] + 0.25 * ext[1]
    quad = np.array([[mid[0] - half, y, mid[2] - half], [mid[0] + half, y, mid[2] - half], [mid[0] + half, y, mid[2] + half],
                     [mid[0] - half, y, mid[2] + half]])
    nv, nt, nm = len(vx), len(a["tri_material"]), sd.n_materials
    keep = {
        "vx": np.concatenate([vx, quad[:, 0]]), "vy": np.concatenate([vy, quad[:, 1]]), "vz": np.concatenate([vz, quad[:, 2]]),
        "idx": np.concatenate([a["tri_indices"], np.array([nv, nv + 1, nv + 2, nv, nv + 2, nv + 3], dtype=np.int32)]),
        "uv": np.concatenate([a["tri_uv"], np.array([0.0, 0, 1, 0, 1, 1, 0, 0, 1, 1, 0, 1])]),
        "tm": np.concatenate([a["tri_material"], np.array([nm, nm], dtype=np.int32)]),
        "fv": a["floor_vertices"], "fuv": a["floor_uv"], "fm": a["floor_material"],
    }
    keep = {k: np.ascontiguousarray(v) for k, v in keep.items()}
    mats = (abi.Material * (nm + 1))()
    for i in range(nm):
        ctypes.memmove(ctypes.byref(mats[i]), ctypes.byref(sd.materials[i]), ctypes.sizeof(abi.Material))
    texs = (abi.Texture * (sd.n_textures + 1))()
    for i in range(sd.n_textures):
        ctypes.memmove(ctypes.byref(texs[i]), ctypes.byref(sd.textures[i]), ctypes.sizeof(abi.Texture))
    texs[sd.n_textures].kind = abi.PTX_TEX_SOLID
    mats[nm].kind, mats[nm].texture = abi.PTX_MAT_LAMBERTIAN, sd.n_textures
    mats[nm].emit[:] = [emit, emit, emit]
    d = abi.SceneDesc()
    assert sd.n_spheres == 0
    d.n_vertices, d.n_triangles = nv + 4, nt + 2
    d.vertex_x, d.vertex_y, d.vertex_z = _dp(keep["vx"]), _dp(keep["vy"]), _dp(keep["vz"])
    d.tri_indices, d.tri_uv, d.tri_material = _ip(keep["idx"]), _dp(keep["uv"]), _ip(keep["tm"])
    d.n_floor_triangles = sd.n_floor_triangles
    if sd.n_floor_triangles:
        d.floor_vertices, d.floor_uv, d.floor_material = _dp(keep["fv"]), _dp(keep["fuv"]), _ip(keep["fm"])
    d.n_materials, d.materials, d.n_textures, d.textures = nm + 1, mats, sd.n_textures + 1, texs
    d.camera, d.background = sd.camera, sd.background
    d.leaf_kind, d.length_cutoff, d.num_bins, d.reserved = sd.leaf_kind, sd.length_cutoff, sd.num_bins, sd.reserved
    return d, (keep, mats, texs, src)
