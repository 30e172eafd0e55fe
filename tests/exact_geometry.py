"""An exact, oracle-independent reference for "the closest hit of a ray under the reference's rules".

Plain helper module (not a conftest) shared by tests/test_exact_geometry.py (the CPU oracle) and
tests/test_gpu_exact_geometry.py (ptx_intersect_rays).  Nothing here calls the oracle or the product: the scene is
read from the ptx_scene_desc arrays and every hit is decided from the geometry by brute force over the build list.

The rules restated (no tree is involved; the closest hit is a property of the geometry):

* Triangle.intersect, Moller-Trumbore (triangle/triangle.ml:74-98): |det| < 1e-6 (absolute, the binary64 value of the
  literal) is a miss; a hit needs 0 <= u, u <= 1, 0 <= v and u + v <= 1, all inclusive, and t_min <= t <= t_max with
  t_min = 0, t_max = max_finite.  The reference forms e1 = b - a, e2 = c - a and tvec = o - a in binary64.
* Sphere.intersect (sphere/src/sphere.ml:35-54) and its packet twin (sphere-intersect-rs/src/lib.rs:103-240): with
  c = |center - o|^2 - r^2 > 0 (origin outside) t = c / q, the near root, so a sphere behind the ray is a miss;
  otherwise t = q / a with q = b' + sign(b') sqrt(a * discrim): the far root for b' >= 0 and a negative root (a miss)
  for b' < 0.  discrim < 0 is a miss.  Ties inside a packet go to the last index (`<=`); ties in general depend on
  the tree, so a tied ray is never robust.
* Floor triangles (ganesha/bin/main.ml:247-256, 286-298) are tested before the tree, in order, and the FIRST that
  hits clips the tree's t_max (inclusive: a tree hit at exactly that t wins).  Numbering as ptx_intersect_rays
  documents it (include/ptx.h): [triangles] @ [spheres] is the build list, floor triangle i is n_tri + n_sph + i.

Robustness.  Every decision quantity q of a ray (det against +-1e-6, u, 1 - u, v, 1 - u - v and t against 0 for a
triangle; discrim, c, b' and t against 0 for a sphere; the separation between the winner's t and every competitor's)
is computed exactly and carries a rigorous forward-error bound E(q) on |q_binary64 - q_exact|.  A ray is robust only
if |q_exact| > 4 E(q) for every quantity its answer depends on; other rays are dropped and counted, never compared.

The bound (class EV) is propagated operation by operation in the order the reference evaluates, with u = 2^-53,
eta = 2^-1074 (one rounding in the subnormal range) and gamma_k = k u / (1 - k u):

* operands: |x_ref - x_exact| <= e_x and |x_numpy - x_exact| <= e_x; A_x = |x_numpy| + 2 e_x bounds |x_exact|,
  |x_ref| and |x_numpy| alike;
* x +- y:   e = e_x + e_y + u (|x +- y| + 2 e_x + 2 e_y) + eta   (gamma_1 times the sum the operation forms);
* x * y:    e = A_x e_y + A_y e_x + u A_x A_y + eta;
* fma(x, y, z) = x y + z: e = A_x e_y + A_y e_x + e_z + gamma_2 (A_x A_y + |x y + z|) + 2 eta -- this covers both
  the fused evaluation (one rounding) and numpy's unfused one (two);
* x / y:    with L = |y_numpy| - 2 e_y > 0 (else e = inf): e = e_x / L + A_x e_y / L^2 + u A_x / L + eta;
* sqrt(x):  e = e_x / sqrt(x_numpy - e_x) (sqrt(e_x) if that is not positive) + u sqrt(A_x) + eta;
* a = |d|^2, whose terms are all non-negative: e = gamma_5 sum d_i^2 + 3 eta, valid for the left-associated
  unfused sum of the packet code (lib.rs:38-40) and the fma chain of V3.quadrance alike;
* b' / a is bounded as b' * fl(1 / a) and q / a as q * fl(1 / a) (the packet code's order; the bound is larger than
  the one for a single division, so it covers sphere.ml's order too).

e1 = b - a, e2 = c - a and tvec = o - a are operations on exact inputs, so their error is u |b - a| etc., and that
error propagates through the cross and dot products like any other.  Every bound is finally multiplied by
1 + 2^-40 for the rounding of the bound's own arithmetic.  The t bound of a ray is E(t) of its winner: the
derivation above applied to t = fl(1 / det) * dot(e2, qvec) (triangle) or c / q, q * fl(1 / a) (sphere).

Exact arithmetic: fractions.Fraction for every rational quantity (all of them but the sphere's t); the sphere's t
needs a square root and is evaluated with mpmath at 80 digits (its error, < 1e-75 relative, is added to the bound).

Speed: a conservative cull (the line misses a ball around the primitive by a margin larger than any binary64 error
of the primitive's test, see `_cull`), then the binary64 pre-pass above vectorised in numpy for the survivors; only
pairs inside a generous window (within 1e-6 of a barycentric boundary, 1e-6 relative of the det threshold, 1e8 E of
any other boundary, or within 1e-6 relative of the ray's float best t) are decided in exact arithmetic.  Everything
outside the window is decided by the pre-pass with a margin of more than 8 E, i.e. robustly.
"""
import ctypes as C
from fractions import Fraction

import numpy as np
import pytest

mpmath = pytest.importorskip("mpmath")

U = 2.0 ** -53
ETA = 2.0 ** -1074
SAFE = 1.0 + 2.0 ** -40
EPS_DET = 1e-6  # triangle.ml:75
GAMMA5 = 5 * U / (1 - 5 * U)
_MP = mpmath.MPContext()
_MP.dps = 80

HIT, MISS, UNSURE = 1, 0, -1


# ---------------------------------------------------------------- scene descriptions
def make_desc(abi, spheres=(), tris=(), leaf_kind=1, cutoff=4, mats=None, num_bins=32, tri_uv=None, materials=None,
              textures=None, background=None):
    """spheres: (x, y, z, r, mat); tris: (a, b, c, mat) with 3-vectors.  Returns (desc, keepalive).
    Optional (the defaults build the same description as before): tri_uv, 6 numbers per triangle (ta, tb, tc); materials,
    (kind, texture, index, emit3) each; textures, (kind, width, height, even3, odd3) each; background, "sky" or "black"."""
    keep = []
    d = abi.SceneDesc()
    sp = np.array([s[:4] for s in spheres], dtype=np.float64).reshape(-1, 4)
    cols = [np.ascontiguousarray(sp[:, k]) for k in range(4)]
    sm = np.array([s[4] for s in spheres], dtype=np.int32)
    keep += cols + [sm]
    d.n_spheres = len(spheres)
    if len(spheres):
        d.sphere_x, d.sphere_y, d.sphere_z, d.sphere_r = [c.ctypes.data_as(abi.c_double_p) for c in cols]
        d.sphere_material = sm.ctypes.data_as(abi.c_int32_p)
    if len(tris):
        v = np.array([p for t in tris for p in t[:3]], dtype=np.float64).reshape(-1, 3)
        vc = [np.ascontiguousarray(v[:, k]) for k in range(3)]
        idx = np.arange(3 * len(tris), dtype=np.int32)
        uv = np.tile(np.array([0.0, 0.0, 1.0, 0.0, 1.0, 1.0]), len(tris)) if tri_uv is None else \
            np.ascontiguousarray(tri_uv, dtype=np.float64).reshape(6 * len(tris))
        tm = np.array([t[3] for t in tris], dtype=np.int32)
        keep += vc + [idx, uv, tm]
        d.n_vertices, d.n_triangles = len(v), len(tris)
        d.vertex_x, d.vertex_y, d.vertex_z = [c.ctypes.data_as(abi.c_double_p) for c in vc]
        d.tri_indices = idx.ctypes.data_as(abi.c_int32_p)
        d.tri_uv = uv.ctypes.data_as(abi.c_double_p)
        d.tri_material = tm.ctypes.data_as(abi.c_int32_p)
    M = (abi.Material * 3)()
    T = (abi.Texture * 2)()
    T[0].kind = abi.PTX_TEX_SOLID
    T[0].even[:] = [0.8, 0.5, 0.3]
    T[1].kind = abi.PTX_TEX_CHECKER
    T[1].width, T[1].height = 8, 16
    T[1].even[:] = [0.9, 0.9, 0.9]
    T[1].odd[:] = [0.1, 0.2, 0.3]
    M[0].kind, M[0].texture = abi.PTX_MAT_LAMBERTIAN, 1
    M[1].kind, M[1].texture = abi.PTX_MAT_METAL, 0
    M[2].kind, M[2].index = abi.PTX_MAT_DIELECTRIC, 1.5
    if materials is not None:
        M = (abi.Material * len(materials))()
        for m, (kind, tex, index, emit) in zip(M, materials):
            m.kind, m.texture, m.index = kind, tex, index
            m.emit[:] = list(emit)
    if textures is not None:
        T = (abi.Texture * len(textures))()
        for t, (kind, w, h, even, odd) in zip(T, textures):
            t.kind, t.width, t.height = kind, w, h
            t.even[:], t.odd[:] = list(even), list(odd)
    keep += [M, T]
    d.n_materials, d.materials, d.n_textures, d.textures = len(M), M, len(T), T
    d.camera.lower_left_x, d.camera.lower_left_y, d.camera.view_x, d.camera.view_y = -1.0, -0.5, 2.0, 1.0
    d.background.kind = abi.PTX_BG_BLACK if background == "black" else abi.PTX_BG_SKY
    d.background.horizon[:] = [1.0, 1.0, 1.0]
    d.background.zenith[:] = [0.5, 0.7, 1.0]
    d.leaf_kind, d.length_cutoff, d.num_bins = leaf_kind, cutoff, num_bins
    return d, keep


class Geometry:
    """The build list and the floor of a ptx_scene_desc, as numpy arrays: tri_a/b/c (n_tri, 3), sph_c (n_sph, 3),
    sph_r (n_sph,), floor_a/b/c (n_floor, 3)."""

    def __init__(self, desc_ptr):
        d = desc_ptr.contents if hasattr(desc_ptr, "contents") else desc_ptr

        def arr(p, n):
            return np.ctypeslib.as_array(p, shape=(n,)).copy() if n else np.zeros(0)

        nt, ns, nf = d.n_triangles, d.n_spheres, d.n_floor_triangles
        if nt:
            vx, vy, vz = (arr(p, d.n_vertices) for p in (d.vertex_x, d.vertex_y, d.vertex_z))
            idx = np.ctypeslib.as_array(d.tri_indices, shape=(3 * nt,)).reshape(nt, 3)
            verts = np.stack([vx, vy, vz], axis=1)
            self.tri_a, self.tri_b, self.tri_c = (verts[idx[:, k]] for k in range(3))
        else:
            self.tri_a = self.tri_b = self.tri_c = np.zeros((0, 3))
        if ns:
            self.sph_c = np.stack([arr(d.sphere_x, ns), arr(d.sphere_y, ns), arr(d.sphere_z, ns)], axis=1)
            self.sph_r = arr(d.sphere_r, ns)
        else:
            self.sph_c, self.sph_r = np.zeros((0, 3)), np.zeros(0)
        if nf:
            fv = np.ctypeslib.as_array(d.floor_vertices, shape=(9 * nf,)).reshape(nf, 3, 3).copy()
            self.floor_a, self.floor_b, self.floor_c = fv[:, 0], fv[:, 1], fv[:, 2]
        else:
            self.floor_a = self.floor_b = self.floor_c = np.zeros((0, 3))
        self.n_tri, self.n_sph, self.n_floor = nt, ns, nf
        self.n_prims = nt + ns
        self.leaf_kind, self.length_cutoff = d.leaf_kind, d.length_cutoff
        self.num_bins = d.num_bins if d.num_bins > 0 else 32

    def prim_boxes(self):
        """Triangle.bbox (componentwise min / max of the vertices, triangle.ml:67-72) and Sphere.bbox
        (center + (-r), center + r, sphere.ml:16-19) in build-list order: (n_prims, 6)."""
        lo = np.minimum(np.minimum(self.tri_a, self.tri_b), self.tri_c)
        hi = np.maximum(np.maximum(self.tri_a, self.tri_b), self.tri_c)
        r = self.sph_r[:, None]
        slo, shi = self.sph_c + (-r), self.sph_c + r
        return np.concatenate([np.concatenate([lo, hi], axis=1), np.concatenate([slo, shi], axis=1)])


# ---------------------------------------------------------------- binary64 forward-error bounds (see the module docstring)
class EV:
    """A binary64 quantity evaluated in numpy (v) with a bound e on |v_ref - exact| and on |v - exact|."""
    __slots__ = ("v", "e")

    def __init__(self, v, e=None):
        self.v = np.asarray(v, dtype=np.float64)
        self.e = np.zeros_like(self.v) if e is None else e

    def mag(self):
        return np.abs(self.v) + 2.0 * self.e

    def __neg__(self):
        return EV(-self.v, self.e)


def _fin(e):
    return e * SAFE


def ev_add(x, y, sign=1.0):
    v = x.v + sign * y.v
    pe = x.e + y.e
    return EV(v, _fin(pe + U * (np.abs(v) * (1 + 2 * U) + 2 * pe + 2 * ETA) + ETA))


def ev_sub(x, y):
    return ev_add(x, y, -1.0)


def ev_mul(x, y):
    ax, ay = x.mag(), y.mag()
    return EV(x.v * y.v, _fin(ax * y.e + ay * x.e + U * ax * ay + ETA))


def ev_fma(x, y, z):
    ax, ay = x.mag(), y.mag()
    v = x.v * y.v + z.v
    pe = ax * y.e + ay * x.e + z.e
    p = ax * ay
    s = np.abs(v) * (1 + 2 * U) + U * p + 2 * pe + 2 * ETA
    return EV(v, _fin(pe + 2 * U / (1 - 2 * U) * (p + s) + 3 * ETA))


def ev_div(x, y):
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        lo = np.abs(y.v) - 2.0 * y.e
        ok = lo > 0
        L = np.where(ok, lo, 1.0)
        ax = x.mag()
        e = x.e / L + ax * y.e / (L * L) + U * ax / L + ETA
        return EV(x.v / np.where(y.v == 0, np.nan, y.v), np.where(ok, _fin(e), np.inf))


def ev_sqrt(x):
    with np.errstate(invalid="ignore", divide="ignore"):
        lo = x.v - x.e
        pe = np.where(lo > 0, x.e / np.sqrt(np.where(lo > 0, lo, 1.0)), np.sqrt(x.e))
        return EV(np.sqrt(np.maximum(x.v, 0.0)), _fin(pe + U * np.sqrt(x.mag()) + ETA))


def ev_dot(p, q):  # V3.dot, affine.ml:60: fma x (fma y (z * z'))
    return ev_fma(p[0], q[0], ev_fma(p[1], q[1], ev_mul(p[2], q[2])))


def ev_cross(p, q):  # V3.cross, affine.ml:70-73: h w x y z = fma w x (-(y * z))
    def h(w, x, y, z):
        return ev_fma(w, x, -ev_mul(y, z))
    a, b, c = p
    d, e, f = q
    return (h(b, f, c, e), h(c, d, a, f), h(a, e, b, d))


def _cols(a):
    return [EV(np.ascontiguousarray(a[..., k])) for k in range(3)]


@np.errstate(all="ignore")  # degenerate pairs give inf / NaN values whose bounds are inf: never robust
def tri_prepass(A, B, Cc, O, D):
    """Triangle.intersect in binary64 with bounds; every argument (m, 3).  Returns a dict of EVs."""
    a, b, c, o, d = _cols(A), _cols(B), _cols(Cc), _cols(O), _cols(D)
    e1 = [ev_sub(b[k], a[k]) for k in range(3)]
    e2 = [ev_sub(c[k], a[k]) for k in range(3)]
    pvec = ev_cross(d, e2)
    det = ev_dot(e1, pvec)
    inv = ev_div(EV(np.ones_like(det.v)), det)
    tvec = [ev_sub(o[k], a[k]) for k in range(3)]
    u = ev_mul(inv, ev_dot(tvec, pvec))
    qvec = ev_cross(tvec, e1)
    v = ev_mul(inv, ev_dot(d, qvec))
    s = ev_add(u, v)
    t = ev_mul(inv, ev_dot(e2, qvec))
    return {"det": det, "u": u, "v": v, "s": s, "t": t}


@np.errstate(all="ignore")
def sph_prepass(Cn, R, O, D):
    """Sphere.intersect / the packet body in binary64 with bounds (the larger of the two evaluation orders)."""
    cc, o, d = _cols(Cn), _cols(O), _cols(D)
    r = EV(np.asarray(R, dtype=np.float64))
    f = [ev_sub(cc[k], o[k]) for k in range(3)]
    bp = ev_dot(f, d)
    a2 = d[0].v * d[0].v + d[1].v * d[1].v + d[2].v * d[2].v
    a = EV(a2, _fin(GAMMA5 * a2 + 3 * ETA))
    r2 = ev_mul(r, r)
    c = ev_sub(ev_dot(f, f), r2)
    inv_a = ev_div(EV(np.ones_like(a.v)), a)
    s = ev_mul(bp, inv_a)
    w = [ev_fma(d[k], s, -f[k]) for k in range(3)]
    disc = ev_sub(r2, ev_dot(w, w))
    sq = ev_sqrt(ev_mul(a, disc))
    sign = np.where(bp.v >= 0, 1.0, -1.0)
    q = ev_add(bp, EV(sign * sq.v, sq.e))
    t_out = ev_div(c, q)
    t_in = ev_mul(q, inv_a)
    outside = c.v > 0
    t = EV(np.where(outside, t_out.v, t_in.v), np.where(outside, t_out.e, t_in.e))
    return {"disc": disc, "c": c, "bp": bp, "t": t}


# ---------------------------------------------------------------- the same quantities in exact arithmetic
def _F(x):
    return Fraction(float(x))


def _fdot(p, q):
    return p[0] * q[0] + p[1] * q[1] + p[2] * q[2]


def _fcross(p, q):
    return (p[1] * q[2] - p[2] * q[1], p[2] * q[0] - p[0] * q[2], p[0] * q[1] - p[1] * q[0])


def tri_exact(a, b, c, o, d):
    """Exact det, u, v, 1 - u - v and t of Moller-Trumbore for the TRUE triangle (e1 = b - a exactly)."""
    a, b, c, o, d = ([_F(x) for x in p] for p in (a, b, c, o, d))
    e1 = [b[k] - a[k] for k in range(3)]
    e2 = [c[k] - a[k] for k in range(3)]
    pvec = _fcross(d, e2)
    det = _fdot(e1, pvec)
    if det == 0:
        return {"det": det, "u": None, "v": None, "w": None, "t": None}
    tvec = [o[k] - a[k] for k in range(3)]
    qvec = _fcross(tvec, e1)
    u = _fdot(tvec, pvec) / det
    v = _fdot(d, qvec) / det
    return {"det": det, "u": u, "v": v, "w": 1 - u - v, "t": _fdot(e2, qvec) / det}


def sph_exact(cn, r, o, d):
    """Exact discrim = r^2 - |f - d b'/a|^2 = r^2 - |f|^2 + b'^2 / a, c, b' (rationals) and t (mpmath, 80 digits)."""
    cn, o, d = ([_F(x) for x in p] for p in (cn, o, d))
    r = _F(r)
    f = [cn[k] - o[k] for k in range(3)]
    bp = _fdot(f, d)
    a = _fdot(d, d)
    ff = _fdot(f, f)
    c = ff - r * r
    disc = r * r - ff + bp * bp / a
    t = None
    if disc >= 0:
        with _MP.workdps(80):
            sq = _MP.sqrt(_mpq(bp * bp - a * c))
            q = _mpq(bp) + (sq if bp >= 0 else -sq)
            t = (_mpq(c) / q if q != 0 else _MP.inf) if c > 0 else q / _mpq(a)
    return {"disc": disc, "c": c, "bp": bp, "t": t}


def _robust(q, e):
    """+1 / -1: q exactly positive / negative by more than 4 e; 0: not robust."""
    if q is None or not np.isfinite(e):
        return 0
    m = 4 * Fraction(float(e))
    return 1 if q > m else (-1 if q < -m else 0)


def tri_status_exact(ex, ev, i):
    """HIT / MISS / UNSURE from exact quantities and the bounds of pair i; the near-edge ratio of a hit."""
    det = ex["det"]
    g = _robust(abs(det) - Fraction(EPS_DET), ev["det"].e[i])
    if g < 0:
        return MISS, None
    if g == 0:
        return UNSURE, None
    qs = [(ex["u"], ev["u"].e[i]), (1 - ex["u"], ev["u"].e[i]), (ex["v"], ev["v"].e[i]), (ex["w"], ev["s"].e[i]),
          (ex["t"], ev["t"].e[i])]
    rs = [_robust(q, e) for q, e in qs]
    if min(rs) < 0:
        return MISS, None
    if min(rs) == 0:
        return UNSURE, None
    ratio = min(float(abs(q) / Fraction(float(e))) if e > 0 else np.inf for q, e in qs[:4])
    return HIT, ratio


def sph_status_exact(ex, ev, i):
    g = _robust(ex["disc"], ev["disc"].e[i])
    if g < 0:
        return MISS, None
    if g == 0 or _robust(ex["c"], ev["c"].e[i]) == 0 or _robust(ex["bp"], ev["bp"].e[i]) == 0:
        return UNSURE, None
    te = ev["t"].e[i]
    if ex["t"] is None or not np.isfinite(te):
        return UNSURE, None
    m = 4 * te
    if ex["t"] > m:
        return HIT, float(ex["disc"] / Fraction(float(ev["disc"].e[i]))) if ev["disc"].e[i] > 0 else np.inf
    return (MISS, None) if ex["t"] < -m else (UNSURE, None)


# ---------------------------------------------------------------- pre-pass classification
def _tri_clear(ev):
    """Per pair: -1 clearly a miss, +1 clearly a hit, 0 inside the window (decided exactly)."""
    det = ev["det"]
    with np.errstate(invalid="ignore"):
        g = np.abs(det.v) - EPS_DET
        wdet = np.maximum(EPS_DET * 1e-6, 8 * det.e)
        qs = [(ev["u"].v, ev["u"].e, 1.0), (1 - ev["u"].v, ev["u"].e, 1.0), (ev["v"].v, ev["v"].e, 1.0),
              (1 - ev["s"].v, ev["s"].e, 1.0), (ev["t"].v, ev["t"].e, 0.0)]
        neg = np.zeros(det.v.shape, bool)
        pos = np.ones(det.v.shape, bool)
        for q, e, scale in qs:
            w = np.maximum(1e-6 * scale, np.where(scale > 0, 8 * e, 1e8 * e))
            neg |= q < -w
            pos &= q > w
        out = np.zeros(det.v.shape, np.int8)
        out[(g > wdet) & pos] = 1
        out[(g < -wdet) | ((g > wdet) & neg)] = -1
    return out


def _sph_clear(ev):
    with np.errstate(invalid="ignore"):
        d, c, bp, t = ev["disc"], ev["c"], ev["bp"], ev["t"]
        dn = d.v < -1e8 * d.e
        ok = (d.v > 1e8 * d.e) & (np.abs(c.v) > 1e8 * c.e) & (np.abs(bp.v) > 1e8 * bp.e) & np.isfinite(t.e)
        out = np.zeros(d.v.shape, np.int8)
        out[ok & (t.v > 1e8 * t.e)] = 1
        out[dn | (ok & (t.v < -1e8 * t.e))] = -1
    return out


def _slack(L_plus_R, scale_e, dn):
    return 2.0 ** -20 * L_plus_R + 1e3 * scale_e * L_plus_R * dn


def _cull_flat(centers, radii, scale_e, O, D, chunk=64):
    ref = centers.mean(axis=0)
    Cn = centers - ref
    rows, cols = [], []
    cn2 = (Cn * Cn).sum(axis=1)
    for s in range(0, len(O), chunk):
        o = O[s:s + chunk] - ref
        d = D[s:s + chunk]
        dn = np.sqrt((d * d).sum(axis=1))
        du = d / dn[:, None]
        od = (o * du).sum(axis=1)
        oo = (o * o).sum(axis=1)
        dist2 = cn2[:, None] - 2 * (Cn @ o.T) + oo[None, :]  # |c - o|^2
        along = Cn @ du.T - od[None, :]
        perp2 = dist2 - along * along
        rr = radii[:, None] + _slack(np.sqrt(np.maximum(dist2, 0.0)) + radii[:, None], scale_e[:, None], dn[None, :])
        fuzz = 1e-13 * (cn2[:, None] + oo[None, :])  # binary64 error of perp2 and along: < 40 u (|c|^2 + |o|^2)
        keep = (perp2 <= rr * rr + fuzz) & (along >= -rr - np.sqrt(fuzz))
        i, j = np.nonzero(keep)
        rows.append(j + s)
        cols.append(i)
    return np.concatenate(rows), np.concatenate(cols)


def _cull_pairs(centers, radii, scale_e, O, D, rays, prims):
    v = centers[prims] - O[rays]
    d = D[rays]
    dn = np.sqrt((d * d).sum(axis=1))
    along = (v * d).sum(axis=1) / dn
    v2 = (v * v).sum(axis=1)
    perp2 = v2 - along * along
    rr = radii[prims] + _slack(np.sqrt(v2) + radii[prims], scale_e[prims], dn)
    fuzz = 1e-13 * v2
    keep = (perp2 <= rr * rr + fuzz) & (along >= -rr - np.sqrt(fuzz))
    return rays[keep], prims[keep]


def _cull(centers, radii, scale_e, O, D, group=32):
    """Pairs (ray, primitive) whose half-line passes within radius + margin of the primitive's ball.  The margin is,
    per pair, 2^-20 (|o - center| + radius) + 1e3 scale_e (|o - center| + radius) |d|: far above the binary64 error of
    the primitive's test (for a triangle |det| >= 1e-6 makes the barycentric error <= ~30 u |tvec| |d| |e|^2 / 1e-6,
    i.e. a distance of that times |e|, and scale_e = u |e|^3 / 1e-6; for a sphere the discriminant's error is
    ~10 u (|f|^2 + r^2)), so a culled primitive is missed both exactly and in binary64.  Large lists are culled by
    groups of `group` primitives first (consecutive in Morton order; a group's ball encloses its members' balls and
    carries their largest margin, so the group test is conservative), then primitive by primitive.  This only
    prunes: every primitive a ray can hit is tested."""
    if len(centers) == 0:
        return np.zeros(0, np.int64), np.zeros(0, np.int64)
    if len(centers) <= 4 * group * 32:
        return _cull_flat(centers, radii, scale_e, O, D)
    lo, hi = centers.min(0), centers.max(0)
    q = ((centers - lo) / np.maximum(hi - lo, 1e-300) * 1023).astype(np.int64)
    code = np.zeros(len(centers), np.int64)
    for bit in range(10):
        for ax in range(3):
            code |= ((q[:, ax] >> bit) & 1) << (3 * bit + ax)
    order = np.argsort(code, kind="stable")
    n_g = (len(order) + group - 1) // group
    pad = np.concatenate([order, np.full(n_g * group - len(order), order[-1])]).reshape(n_g, group)
    gc = centers[pad].mean(axis=1)
    gr = (np.sqrt(((centers[pad] - gc[:, None]) ** 2).sum(-1)) + radii[pad]).max(1) * (1 + 1e-9)
    gs = scale_e[pad].max(1)
    rays, groups = _cull_flat(gc, gr, gs, O, D)
    rays = np.repeat(rays, group)
    prims = pad[groups].reshape(-1)
    rays, prims = _cull_pairs(centers, radii, scale_e, O, D, rays, prims)
    u = np.unique(rays * len(centers) + prims)  # the padding repeats the last primitive
    return u // len(centers), u % len(centers)


class Reference:
    """Brute-force closest hits of a Geometry; `closest(O, D)` returns a Result."""

    def __init__(self, geo):
        self.g = geo
        A, B, Cc = geo.tri_a, geo.tri_b, geo.tri_c
        cen = (A + B + Cc) / 3.0
        rad = np.sqrt(np.maximum(np.maximum(((A - cen) ** 2).sum(1), ((B - cen) ** 2).sum(1)), ((Cc - cen) ** 2).sum(1)))
        rad = rad * (1 + 1e-9) + 1e-300
        e2 = np.maximum(np.maximum(((B - A) ** 2).sum(1), ((Cc - A) ** 2).sum(1)), ((Cc - B) ** 2).sum(1))
        self.tri_cull = (cen, rad, U * e2 * np.sqrt(e2) / EPS_DET)
        self.sph_cull = (geo.sph_c, geo.sph_r * (1 + 1e-9) + 1e-300, np.zeros(geo.n_sph))

    def closest(self, O, D):
        O = np.ascontiguousarray(O, dtype=np.float64)
        D = np.ascontiguousarray(D, dtype=np.float64)
        n = len(O)
        g = self.g
        # per ray: lists of (t_exact, e_t, prim) of robust hits, (t, e) of undecided pairs, clear far hits
        hits = [[] for _ in range(n)]
        unsure = [[] for _ in range(n)]
        ratio = {}
        far = np.full(n, np.inf)
        far_e = np.zeros(n)
        cand_pairs = 0

        def run(kind, rays, idx, base):
            nonlocal cand_pairs
            if len(rays) == 0:
                return
            if kind == "tri":
                ev = tri_prepass(g.tri_a[idx], g.tri_b[idx], g.tri_c[idx], O[rays], D[rays])
                clear = _tri_clear(ev)
            else:
                ev = sph_prepass(g.sph_c[idx], g.sph_r[idx], O[rays], D[rays])
                clear = _sph_clear(ev)
            t = ev["t"]
            # the float best of every ray over the clear hits and the undecided ones
            best = np.full(n, np.inf)
            best_e = np.zeros(n)
            pot = (clear >= 0) & np.isfinite(t.v) & np.isfinite(t.e)
            np.minimum.at(best, rays[pot], t.v[pot])
            np.maximum.at(best_e, rays[pot], t.e[pot])
            with np.errstate(invalid="ignore"):
                win = np.maximum(1e-6 * np.abs(best[rays]), 8 * (t.e + best_e[rays]))
                near = (clear == 0) | ((clear == 1) & (t.v - best[rays] <= win))
            far_hit = (clear == 1) & ~near
            for k in np.nonzero(far_hit)[0]:
                r = rays[k]
                if t.v[k] - t.e[k] < far[r]:
                    far[r], far_e[r] = t.v[k] - t.e[k], t.e[k]
            for k in np.nonzero(near)[0]:
                cand_pairs += 1
                r, p = rays[k], idx[k]
                if kind == "tri":
                    ex = tri_exact(g.tri_a[p], g.tri_b[p], g.tri_c[p], O[r], D[r])
                    st, rt = tri_status_exact(ex, ev, k)
                    tx = ex["t"]
                else:
                    ex = sph_exact(g.sph_c[p], g.sph_r[p], O[r], D[r])
                    st, rt = sph_status_exact(ex, ev, k)
                    tx = ex["t"]
                if st == HIT:
                    hits[r].append((tx, float(t.e[k]), base + int(p)))
                    ratio[(r, base + int(p))] = rt
                elif st == UNSURE:
                    unsure[r].append((tx, float(t.e[k])))

        rays, idx = _cull(*self.tri_cull, O, D)
        run("tri", rays, idx, 0)
        rays, idx = _cull(*self.sph_cull, O, D)
        run("sph", rays, idx, g.n_tri)

        # floor: every pair exactly (a handful per ray), in order, the first hit wins
        floor_hit = [None] * n
        floor_bad = np.zeros(n, bool)
        if g.n_floor:
            for i in range(g.n_floor):
                m = np.ones(n, bool) if i == 0 else np.array([floor_hit[r] is None and not floor_bad[r] for r in range(n)])
                rs = np.nonzero(m)[0]
                if len(rs) == 0:
                    break
                ev = tri_prepass(np.repeat(g.floor_a[i:i + 1], len(rs), 0), np.repeat(g.floor_b[i:i + 1], len(rs), 0),
                                 np.repeat(g.floor_c[i:i + 1], len(rs), 0), O[rs], D[rs])
                clear = _tri_clear(ev)
                for k, r in enumerate(rs):
                    if clear[k] == -1:
                        continue
                    ex = tri_exact(g.floor_a[i], g.floor_b[i], g.floor_c[i], O[r], D[r])
                    st, rt = tri_status_exact(ex, ev, k)
                    if st == HIT:
                        floor_hit[r] = (ex["t"], float(ev["t"].e[k]), g.n_prims + i)
                        ratio[(r, g.n_prims + i)] = rt
                    elif st == UNSURE:
                        floor_bad[r] = True

        prim = np.full(n, -1, np.int32)
        t_exact = np.full(n, np.nan)
        t_bound = np.zeros(n)
        edge = np.full(n, np.inf)
        robust = np.zeros(n, bool)
        for r in range(n):
            if floor_bad[r]:
                continue
            comp = list(hits[r])
            if floor_hit[r] is not None:
                comp.append(floor_hit[r])
            if np.isfinite(far[r]):
                comp.append((Fraction(float(far[r])), float(far_e[r]), None))
            comp.sort(key=lambda h: _mpq(h[0]))
            if not comp:
                if unsure[r]:
                    continue
                robust[r] = True
                continue
            w = comp[0]
            if w[2] is None:  # the nearest hit lies outside the exact window: not decided here
                continue
            ok = all(_sep(c[0], w[0], c[1] + w[1]) for c in comp[1:])
            ok = ok and all(u[0] is not None and np.isfinite(u[1]) and _sep(u[0], w[0], u[1] + w[1]) for u in unsure[r])
            if not ok:
                continue
            robust[r] = True
            prim[r] = w[2]
            t_exact[r] = float(w[0])
            t_bound[r] = w[1]
            edge[r] = ratio.get((r, w[2]), np.inf)
        return Result(prim, t_exact, t_bound, robust, edge, hits, floor_hit, cand_pairs)


def _sep(t_other, t_win, e):
    """t_other - t_win > 4 e, exactly (t may be a Fraction or an mpmath number)."""
    if t_other is None or t_win is None:
        return False
    if isinstance(t_other, Fraction) and isinstance(t_win, Fraction):
        return t_other - t_win > 4 * Fraction(float(e))
    with _MP.workdps(80):
        diff = _mpq(t_other) - _mpq(t_win)
        slack = _MP.mpf(1e-70) * (abs(_mpq(t_other)) + abs(_mpq(t_win)))
        return diff - slack > 4 * _MP.mpf(float(e))


def _mpq(x):
    if isinstance(x, Fraction):
        return _MP.mpf(x.numerator) / x.denominator
    return x


class Result:
    """prim (-1 miss), t_exact (nearest binary64 of the exact t), t_bound (E(t) of the winner), robust, edge (the
    winner's smallest |q| / E(q) over its barycentric / silhouette quantities; inf for misses)."""

    def __init__(self, prim, t_exact, t_bound, robust, edge, hits, floor_hit, cand_pairs):
        self.prim, self.t_exact, self.t_bound, self.robust, self.edge = prim, t_exact, t_bound, robust, edge
        self.cand_pairs = cand_pairs

    def summary(self, t_got=None):
        n = len(self.prim)
        out = {"rays": n, "robust": int(self.robust.sum()), "hits": int((self.robust & (self.prim >= 0)).sum()),
               "near_edge": int((self.robust & (self.edge <= 100)).sum())}
        if t_got is not None:
            m = self.robust & (self.prim >= 0)
            frac = np.abs(t_got[m] - self.t_exact[m]) / np.maximum(self.t_bound[m], 1e-300)
            out["worst_t_err_over_bound"] = float(frac.max()) if m.any() else 0.0
            out["median_bound_rel"] = float(np.median(self.t_bound[m] / np.abs(self.t_exact[m]))) if m.any() else 0.0
        return out


def compare(res, prim_got, t_got):
    """Assertion messages (empty when the robust rays agree): primitive equal, |t_got - t_exact| <= E(t)."""
    bad = []
    m = res.robust
    wrong = np.nonzero(m & (prim_got != res.prim))[0]
    for r in wrong[:5]:
        bad.append(f"ray {r}: prim {prim_got[r]} (t {t_got[r]!r}), exact {res.prim[r]} (t {res.t_exact[r]!r})")
    if len(wrong):
        bad.append(f"{len(wrong)} robust rays hit the wrong primitive")
    h = m & (res.prim >= 0) & (prim_got == res.prim)
    # |t_got - t_exact| with t_exact rounded to binary64: allow the half ulp of that rounding
    err = np.abs(t_got[h] - res.t_exact[h]) - np.spacing(np.abs(res.t_exact[h])) / 2
    over = np.nonzero(err > res.t_bound[h])[0]
    if len(over):
        k = np.nonzero(h)[0][over[0]]
        bad.append(f"{len(over)} robust hits outside their t bound, e.g. ray {k}: t {t_got[k]!r} exact {res.t_exact[k]!r} "
                   f"bound {res.t_bound[k]:.3e}")
    return bad


# ---------------------------------------------------------------- ray sets
def _unit(v):
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


def _perp(v, rng):
    p = np.cross(v, rng.normal(size=3))
    return p / np.linalg.norm(p)


def make_rays(geo, n, seed, edge_fraction=0.65):
    """Rays aimed at chosen primitives (interior points, and points pushed toward edges / vertices / silhouettes until
    they sit a few bounds above the robustness limit), plus origins outside / between / inside, unnormalised directions,
    zero components, components down to 1e-300 and a subnormal one, and rays that miss.  Returns (O, D)."""
    rng = np.random.default_rng(seed)
    pb = geo.prim_boxes()
    lo, hi = pb[:, :3].min(0), pb[:, 3:].max(0)
    diag = float(np.linalg.norm(hi - lo))  # of the build list: the floor is larger than the scene by far
    mid = (lo + hi) / 2
    n_tri_rays = n * geo.n_tri // max(geo.n_prims, 1) if geo.n_sph else (n if geo.n_tri else 0)
    n_tri_rays = int(n_tri_rays * 0.85)
    n_sph_rays = int((n - n_tri_rays) * 0.85) if geo.n_sph else 0
    n_misc = n - n_tri_rays - n_sph_rays
    O, D, pushed = [], [], []

    def origin_for(P, size):
        k = rng.random()
        if k < 0.6:  # outside: from a few to a few hundred primitive sizes away, at most twice the scene's diagonal
            return P - _unit(rng.normal(size=3)) * min(size * 10.0 ** rng.uniform(0.3, 2.5), 2 * diag)
        if k < 0.9:  # close by, between primitives
            return P - _unit(rng.normal(size=3)) * diag * 10.0 ** rng.uniform(-4, -1)
        return P - _unit(rng.normal(size=3)) * np.linalg.norm(P - mid) * rng.uniform(0.5, 3.0) - (P - mid)

    # --- triangles: interior points, then a share pushed toward an edge / vertex using the pair's own bounds
    if n_tri_rays:
        ks = rng.integers(0, geo.n_tri, n_tri_rays)
        a, b, c = geo.tri_a[ks], geo.tri_b[ks], geo.tri_c[ks]
        bary = rng.dirichlet([1.0, 1.0, 1.0], n_tri_rays)
        P = bary[:, :1] * a + bary[:, 1:2] * b + bary[:, 2:] * c
        size = np.linalg.norm(np.maximum(np.maximum(a, b), c) - np.minimum(np.minimum(a, b), c), axis=1)
        Ot = np.array([origin_for(p, sz) for p, sz in zip(P, size)])
        sc = 10.0 ** rng.uniform(-3, 3, n_tri_rays)  # unnormalised directions
        Dt = (P - Ot) * sc[:, None]
        push = rng.random(n_tri_rays) < edge_fraction / 0.85
        if push.any():
            ev = tri_prepass(a[push], b[push], c[push], Ot[push], Dt[push])
            eu, ev_, es = ev["u"].e, ev["v"].e, ev["s"].e
            mode = rng.integers(0, 5, push.sum())  # u ~ 0, v ~ 0, w ~ 0, vertex a (u, v ~ 0), vertex (w, v ~ 0)
            s1 = 10.0 ** rng.uniform(np.log10(6.0), np.log10(60.0), push.sum())
            s2 = 10.0 ** rng.uniform(np.log10(6.0), np.log10(60.0), push.sum())
            u0, v0 = bary[push, 1].copy(), bary[push, 2].copy()
            u0 = np.where(mode == 0, s1 * eu, u0)
            v0 = np.where(mode == 1, s1 * ev_, v0)
            k2 = np.where(mode == 2, (1 - s1 * es) / (u0 + v0), 1.0)
            u0, v0 = u0 * k2, v0 * k2
            u0 = np.where(mode == 3, s1 * eu, u0)
            v0 = np.where(mode == 3, s2 * ev_, v0)
            v0 = np.where(mode == 4, s1 * ev_, v0)
            u0 = np.where(mode == 4, 1 - v0 - s2 * es, u0)
            # the aim point in exact arithmetic, rounded once: d = (a - o) + u e1 + v e2
            Dp = []
            for aa, bb, cc, oo, uu, vv, ss in zip(a[push], b[push], c[push], Ot[push], u0, v0, sc[push]):
                fa = [_F(x) for x in aa]
                Dp.append([float(_F(ss) * (fa[i] - _F(oo[i]) + _F(uu) * (_F(bb[i]) - fa[i]) + _F(vv) * (_F(cc[i]) - fa[i])))
                           for i in range(3)])
            Dt[push] = np.array(Dp)
        O.append(Ot)
        D.append(Dt)
        pushed.append(push)

    # --- spheres: caps up to grazing; a share pushed to a few bounds above the silhouette
    if n_sph_rays:
        ks = rng.integers(0, geo.n_sph, n_sph_rays)
        Os, Ds = [], []
        for k in ks:
            cn, r = geo.sph_c[k], geo.sph_r[k]
            kind = rng.random()
            if kind < 0.15:  # from inside
                o = cn + _unit(rng.normal(size=3)) * r * rng.uniform(0, 0.9)
                Os.append(o)
                Ds.append(rng.normal(size=3))
                continue
            o = cn + _unit(rng.normal(size=3)) * r * (1 + 10.0 ** rng.uniform(-2, 1.5))
            if kind < 0.2:  # sphere behind the ray
                Os.append(o)
                Ds.append(o - cn + 0.1 * r * rng.normal(size=3))
                continue
            L = cn - o
            p = _perp(L, rng)
            rho = r * np.sqrt(rng.uniform(0, 1))
            Os.append(o)
            Ds.append(L + p * rho * np.linalg.norm(L) / np.sqrt(max(L @ L - rho * rho, 1e-300)))
        Os, Ds = np.array(Os), np.array(Ds) * (10.0 ** rng.uniform(-3, 3, n_sph_rays))[:, None]
        push = rng.random(n_sph_rays) < edge_fraction / 0.85
        if push.any():
            ev = sph_prepass(geo.sph_c[ks[push]], geo.sph_r[ks[push]], Os[push], Ds[push])
            s = 10.0 ** rng.uniform(np.log10(6.0), np.log10(60.0), push.sum())
            new = []
            for j, (k, o) in enumerate(zip(ks[push], Os[push])):
                cn, r = geo.sph_c[k], geo.sph_r[k]
                L = cn - o
                a = float(Ds[push][j] @ Ds[push][j])
                rho_t2 = r * r - s[j] * ev["disc"].e[j]
                if rho_t2 <= 0 or L @ L <= r * r:
                    new.append(Ds[push][j])
                    continue
                rho_t = np.sqrt(rho_t2)
                p = _perp(L, rng)
                rho = rho_t * np.linalg.norm(L) / np.sqrt(L @ L - rho_t2)
                new.append((L + p * rho) * np.sqrt(a / (L @ L + rho * rho)))
            Ds[push] = np.array(new)
        O.append(Os)
        D.append(Ds)
        pushed.append(push)

    # --- the rest: random origins and directions (many miss), rays through the middle, rays pointing away
    if n_misc:
        Om = mid + rng.normal(size=(n_misc, 3)) * diag
        Dm = rng.normal(size=(n_misc, 3))
        away = rng.random(n_misc) < 0.3
        Dm[away] = Om[away] - mid
        O.append(Om)
        D.append(Dm * (10.0 ** rng.uniform(-3, 3, n_misc))[:, None])
        pushed.append(np.zeros(n_misc, bool))
    O, D, pushed = np.concatenate(O), np.concatenate(D), np.concatenate(pushed)
    perm = rng.permutation(len(O))
    O, D, pushed = O[perm], D[perm], pushed[perm]
    # modifiers on the rays not pushed to an edge: axis-aligned directions, tiny components
    k = rng.random(len(O))
    for j in np.nonzero((k < 0.18) & ~pushed)[0]:  # one or two components exactly 0: keep the aim point, move the origin
        P = O[j] + D[j]
        zs = rng.choice(3, size=int(rng.integers(1, 3)), replace=False)
        Dj = D[j].copy()
        Dj[zs] = 0.0 if rng.random() < 0.8 else -0.0
        if not Dj.any():
            continue
        O[j] = P - Dj
        D[j] = Dj
        if rng.random() < 0.4:  # ... or down to 1e-300 (1/d near overflow) and subnormal (1/d = inf)
            D[j][zs[0]] = rng.choice([1e-300, -1e-300, 4e-310, -4e-310])
    return O, D


# ---------------------------------------------------------------- scenes shared by the CPU and GPU tests
def soup(kind, seed, n=300):
    """Random primitives: sizes 1e-3 .. 1e2, a share offset to ~1e4, axis-aligned flat triangles, tiny and large spheres,
    and coincident copies (the rays they tie are not robust and are dropped, never compared)."""
    rng = np.random.default_rng(seed)
    tris, sphs = [], []
    for i in range(n):
        size = 10.0 ** rng.uniform(-3, 2)
        centre = rng.uniform(-50, 50, 3) + (np.array([1e4, -1e4, 1e4]) * rng.uniform(0.5, 1.0) if rng.random() < 0.25 else 0.0)
        tri = kind == "tri" or (kind == "mix" and rng.random() < 0.6)
        if tri:
            if rng.random() < 0.25:  # axis-aligned flat
                ax = int(rng.integers(0, 3))
                pts = centre + rng.normal(size=(3, 3)) * size
                pts[:, ax] = centre[ax]
            else:
                pts = centre + rng.normal(size=(3, 3)) * size
            tris.append((pts[0], pts[1], pts[2], int(rng.integers(0, 3))))
            if rng.random() < 0.03:
                tris.append(tris[-1])
        else:
            r = size if rng.random() < 0.8 else 10.0 ** rng.choice([-4.0, 3.0])
            sphs.append((*centre, r, int(rng.integers(0, 3))))
            if rng.random() < 0.03:
                sphs.append(sphs[-1])
    return sphs, tris


def scene_desc(name, oracle, abi):
    """(desc pointer, keepalive) for a scene name: shirley, shirley_no_simd, cornell, ganesha_3k, ganesha_150k or
    soup-<tri|sph|mix>-<leaf_kind>-<cutoff>-<num_bins>."""
    if name.startswith("soup"):
        _, kind, leaf, cutoff, bins = name.split("-")
        sphs, tris = soup(kind, seed=sum(map(ord, name)))
        d, keep = make_desc(abi, spheres=sphs, tris=tris, leaf_kind=int(leaf), cutoff=int(cutoff), num_bins=int(bins))
        return C.pointer(d), (d, keep)
    od = {"shirley": lambda: oracle.desc_shirley(120, 60), "shirley_no_simd": lambda: oracle.desc_shirley(120, 60, no_simd=True),
          "cornell": lambda: oracle.desc_cornell(64, 64), "ganesha_3k": lambda: oracle.desc_ganesha_like(64, 36, 3000),
          "ganesha_150k": lambda: oracle.desc_ganesha_like(64, 36, 150000)}[name]()
    return od.ptr, od


SCENES = ["shirley", "shirley_no_simd", "cornell", "ganesha_3k", "ganesha_150k",
          "soup-tri-1-1-32", "soup-tri-1-4-4", "soup-tri-1-16-32", "soup-sph-0-16-32", "soup-sph-1-4-4", "soup-sph-0-16-4",
          "soup-mix-1-1-4", "soup-mix-1-4-32", "soup-mix-1-16-32"]

# floors every ray set must clear, so that it cannot drift to easy rays
MIN_ROBUST, MIN_NEAR_EDGE = 0.70, 0.20


def check_floors(name, s):
    msgs = []
    if s["robust"] < MIN_ROBUST * s["rays"]:
        msgs.append(f"{name}: only {s['robust']} of {s['rays']} rays are robust")
    if s["near_edge"] < MIN_NEAR_EDGE * s["rays"]:
        msgs.append(f"{name}: only {s['near_edge']} of {s['rays']} rays lie within 100 bounds of an edge or silhouette")
    return msgs


# ---------------------------------------------------------------- tree invariants (ptx_scene_tree layout, include/ptx.h)
def _unsplittable(boxes, num_bins):
    """Proposal.create finds no split (shape_tree.ml:123-146): the scale num_bins (1 - 1e-6) / (cb_max - cb_min) of the
    centroids' box is not finite on any axis (shape_tree.ml:129-131, 180)."""
    cen = 0.5 * (boxes[:, :3] + boxes[:, 3:])  # Bbox.center, bbox.ml:12
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        scale = float(num_bins) * (1.0 - 1e-6) / (cen.max(0) - cen.min(0))
    return not np.isfinite(scale).any()


def check_tree(geo, bbox, info, order, leaf_size):
    """Messages for every violated invariant (empty list: the tree is sound).  Exact binary64 comparisons throughout."""
    msgs = []
    n = len(info)
    pb = geo.prim_boxes()
    seen = np.zeros(n, np.int64)
    used = np.zeros(geo.n_prims, np.int64)
    stack = [0] if n else []
    while stack:
        k = stack.pop()
        seen[k] += 1
        if seen[k] > 1:
            msgs.append(f"node {k} reached more than once")
            continue
        is_leaf, axis, a, b = (int(x) for x in info[k])
        if is_leaf:
            if a < 0 or b < 0 or a + b > len(order):
                msgs.append(f"leaf {k}: slots [{a}, {a + b}) out of range")
                continue
            slots = order[a:a + b]
            prims = slots[slots >= 0]
            if (slots < -1).any() or (slots >= geo.n_prims).any():
                msgs.append(f"leaf {k}: slot values out of range")
                continue
            if geo.leaf_kind == 0:
                if b > leaf_size:
                    msgs.append(f"leaf {k}: {b} slots > ptx_leaf_size() {leaf_size}")
                if len(prims) and ((slots == -1).sum() >= 4 or (slots[:len(prims)] < 0).any()):
                    msgs.append(f"leaf {k}: padding is not the tail of the last 4-lane group")
            elif (slots == -1).any():
                msgs.append(f"leaf {k}: padding slot in an array leaf")
            if len(prims) == 0:
                msgs.append(f"leaf {k}: empty")
                continue
            used[prims] += 1
            cap = max(geo.length_cutoff, 4)  # Tree.create makes a leaf of <= 4 elements whatever the cutoff (shape_tree.ml:183)
            if len(prims) > cap and not _unsplittable(pb[prims], geo.num_bins):
                msgs.append(f"leaf {k}: {len(prims)} primitives > max(length_cutoff, 4) = {cap} but they can be split")
            box = np.concatenate([pb[prims, :3].min(0), pb[prims, 3:].max(0)])
            if not np.array_equal(box, bbox[k]):
                msgs.append(f"leaf {k}: box {bbox[k].tolist()} != union of its primitives' boxes {box.tolist()}")
        else:
            if axis not in (0, 1, 2):
                msgs.append(f"node {k}: axis {axis}")
            if not (0 < a < n and 0 < b < n):
                msgs.append(f"node {k}: children {a}, {b} out of range")
                continue
            box = np.concatenate([np.minimum(bbox[a, :3], bbox[b, :3]), np.maximum(bbox[a, 3:], bbox[b, 3:])])
            if not np.array_equal(box, bbox[k]):
                msgs.append(f"node {k}: box {bbox[k].tolist()} != union of its children's {box.tolist()}")
            stack += [a, b]
    if n and (seen == 0).any():
        msgs.append(f"{int((seen == 0).sum())} nodes are not reached from the root")
    missing, dup = np.nonzero(used == 0)[0], np.nonzero(used > 1)[0]
    if len(missing):
        msgs.append(f"{len(missing)} primitives are in no leaf, e.g. {missing[:5].tolist()}")
    if len(dup):
        msgs.append(f"{len(dup)} primitives are in more than one slot, e.g. {dup[:5].tolist()}")
    return msgs
