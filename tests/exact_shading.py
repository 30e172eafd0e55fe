"""An oracle-independent restatement of "what happens at a hit" under the reference's rules, evaluated in interval
arithmetic: the camera ray, the sampler, Hit.to_hit of spheres, triangles and floor triangles, Shader_space,
Material.scatter, the textures, the background, the emitter extension and the path loop's accumulation up to two
segments.

Plain helper module (not a conftest) shared by tests/test_exact_shading.py (the CPU oracle) and
tests/test_gpu_exact_shading.py (the kernels).  Nothing here calls the product.  The oracle is called for two inputs
only: the sampler's alpha (orc_lds_alpha, pinned by tests/test_oracle_kat.py) and the binary64 camera ray
(orc_camera_ray), which is itself checked against the restated camera before it is used.  The closest hit of every
segment comes from tests/exact_geometry.py (exact arithmetic, brute force over the build list).

The rules restated, in the reference's operation order (every vector operation is per component):

* Camera.ray (camera.ml:93-102): d = normalize(ll_x + view_x cx, ll_y + view_y cy, -1), origin 0, with cx, cy as
  render_tile forms them (integrator.ml:96-109): cx = (x + L.get 0) * (1 / width), cy = 1 - (y + L.get 1) * (1 / height),
  sampler offset y * width + x + pass * spp (sic: pass times samples per pixel, integrator.ml:98).
* Low_discrepancy_sequence.get (low_discrepancy_sequence.ml:19-20, 33-36): frac(0.5 + alpha_dim * (1 + offset)), with
  frac x = x - trunc x.  The path loop reads dims 2 j and 2 j + 1 at its j-th hit (integrator.ml:38-41).
* V3 (affine.ml): dot = fma x x' (fma y y' (z z')) (:60), cross h w x y z = fma w x (-(y z)) (:70-73), normalize
  v = v * (1 / hypot x (hypot y z)) (:65-68), lerp t v w = v (1 - t) + w t (:63), Color.fma u v w = u v + w (:53).
* Sphere.hit (sphere.ml:21-33, 56-69): p = o + t d, n = normalize(p - center), hit_front = dot(d, n) < 0 (else n is
  negated), tex_coord u = (pi + atan2(-n.z, n.x)) * (1 / (2 pi)), v = acos(-n.y) * (1 / pi).
* Triangle.Hit.to_hit (triangle.ml:24-64): g = normalize(cross(b - a, c - a)), w = 1 - u - v, p = a w + b u + c v,
  tex = ta w + tb u + tc v (left to right), hit_front = dot(d, g) < 0, n = hit_front ? g : -g.  Floor triangles
  (ganesha/bin/main.ml:205-256) are triangles with their own tex coords and material.
* Shader_space.create (shader_space.ml:11-23): z > 1 - 1e-9: rotation (1, 0, 0, 0); z < 1e-9 - 1: (0, 0, 1, 0); else
  Quaternion.normalize (1 + z, y, -x, 0) (quaternion.ml:11-15: q * (1 / hypot (hypot r x) (hypot y z))).
  rotate = Quaternion.transform q v = (q (0, v) q*).v (quaternion.ml:25-42), rotate_inv uses q*; reflect (-x, -y, z);
  refract wi k (:41-49): c = min wi.z 1, perp = k ((0, 0, c) - wi), para = (0, 0, -sqrt |1 - |perp|^2|), perp + para;
  world_ray dir (:51-54): dir' = rotate_inv dir, origin p + 1e-3 dir'; omega_i = rotate(-d) (:66-69);
  unit_square_to_hemisphere u v (:56-64): r = sqrt u, theta = v * 2 * pi, (r cos theta, r sin theta, sqrt(1 - u)).
* Texture.eval (texture.ml:16-31): solid = even; checker: px = to_int(u (width - 1)) land 1, py likewise with v and
  height - 1, even when px = py.
* Material.scatter (material.ml:13-57): Lambertian diffuse with attenuation = texture; Metal: omega_r = reflect omega_i,
  absorb when omega_r.z <= 0, else attenuation a + (1 - a) pow5(1 - omega_i.z) and the ray world_ray omega_r;
  Dielectric: c = clamp(omega_i.z, 0, 1), s = sqrt(1 - c c), ratio = hit_front ? 1 / index : index, reflect when
  ratio s > 1 (TIR) or schlick(c, ratio) > u (schlick c k = r0 + (1 - r0) pow5(1 - c), r0 = ((1 - k) / (1 + k))^2),
  else refract; attenuation 1.
* Pdf (pdf.ml:11-15) and the diffuse branch of the path loop (integrator.ml:45-69): dir = hemisphere(u, v),
  pd = dir.z / pi (0 when dir.z < 0); pd = 0 ends the path with its emission; the attenuation is scaled by pd / pd,
  which is exactly 1 for every finite non-zero pd (the non-finite exit cannot occur: dir.z = sqrt(1 - u) with u in
  [0, 1) is finite and positive whenever it is not 0).
* The background (shirley_spheres/bin/main.ml:104-110): sky = lerp(0.5 (dot(normalize d, (0, 1, 0)) + 1), horizon,
  zenith); black = 0.
* The path loop (integrator.ml:16-75, add_mul a b c = Color.fma b c a): emit0 = 0, attn0 = 1; out of bounces:
  fma(attn0, 0, emit0); a miss: fma(attn0, background, emit0); an absorb (or pd = 0): fma(attn0, emit, emit0); a
  scatter with attenuation k: emit0 <- fma(k, emit0, emit), attn0 <- k attn0.  The emission is the material's
  `emit` (the project's documented emitter extension; black in the reference).

Interval arithmetic.  Every quantity is an interval [lo, hi] of binary64 numbers, vectorised over samples.  Inputs are
binary64 points; the hit's t, u and v enter as [q_exact - E(q), q_exact + E(q)] with E from exact_geometry.  After each
IEEE operation (+ - * / sqrt; fma is evaluated as a product interval followed by a sum interval, which encloses both
the fused and the unfused evaluation) the enclosure of the exact result over the operand intervals is formed from the
endpoints rounded to nearest, widened by one ulp (np.nextafter), and then widened by one more ulp: the result encloses
the exact value of the operation and every binary64 evaluation of it in the same order.  sqrt arguments in these rules
are non-negative by construction (u in [0, 1), 1 - c^2 with c in [0, 1], an absolute value), so the negative part of
an enclosure is dropped before the square root.

The functions csrc/pt_math.h provides (hypot, sin, cos, acos, atan2, pow5) are the one input that rests on a MEASURED
bound, not a proof: their endpoints are evaluated with mpmath at 30 digits, extrema inside the interval are included
(sin / cos critical points; hypot at 0; atan2 over a box, which is monotone along every edge away from the origin and
the branch cut, so its range is attained at the corners), and the result is widened by the bound
tests/test_math.py asserts for that function (1 ulp; atan2 1.5 ulp; pow5 0.5000001 ulp).  acos outside [-1, 1] and
atan2 boxes that touch the branch cut or the origin give an unbounded result (the sample is then never compared).

Enclosures are held to a 99th-percentile relative width of 1e-10, except on three families where the computation is
ill-conditioned (ILL_CONDITIONED below).

Decisions.  A decision (hit_front, both pole tests, checker parity in u and v, metal z <= 0, TIR, Schlick against u, pd
= 0, the sampler's trunc, the hit or miss of a segment) is robust only if its quantity's interval clears the boundary
with margin: |midpoint - boundary| > 4 x half-width (exact_geometry's 4x rule applied to the interval).  A sample is
compared only if every decision its answer depends on is robust and its enclosures are finite; the others are counted.
"""
import ctypes as C

import numpy as np
import pytest

import exact_geometry as X

mpmath = pytest.importorskip("mpmath")

_MP = mpmath.MPContext()
_MP.dps = 30
PI = 3.14159265358979323846  # Float.pi
TWO52 = 2.0 ** -52
MARGIN = 4.0  # exact_geometry's rule
BOUND_ULPS = {"hypot": 1.0, "sin": 1.0, "cos": 1.0, "acos": 1.0, "atan2": 1.5, "pow5": 0.5000001}  # tests/test_math.py
SC_ABSORB, SC_SPECULAR, SC_DIFFUSE = 0, 1, 2
MAT_LAMBERTIAN, MAT_METAL, MAT_DIELECTRIC = 0, 1, 2
# Deliberately wrong variants of the rules: the self-test of tests/test_exact_shading.py must see each one rejected.
MUTANTS = ("offset_1e-4", "rotate_not_inv", "checker_swapped", "index_swapped", "pole_eps_1e-8", "pole_bottom_eps_1e-8",
           "hemisphere_xy_swapped", "add_mul_physical", "checker_width_not_minus_1")


# ---------------------------------------------------------------- intervals
def _dn(x):
    return np.nextafter(x, -np.inf)


def _up(x):
    return np.nextafter(x, np.inf)


class Iv:
    """Vectorised interval [lo, hi] of binary64 numbers."""
    __slots__ = ("lo", "hi")

    def __init__(self, lo, hi=None):
        self.lo = np.asarray(lo, dtype=np.float64)
        self.hi = self.lo if hi is None else np.asarray(hi, dtype=np.float64)

    @staticmethod
    def out(lo, hi):
        """The endpoints rounded to nearest enclose the exact result within one ulp; widen by one more ulp."""
        return Iv(_dn(_dn(lo)), _up(_up(hi)))

    def mid(self):
        with np.errstate(all="ignore"):
            return 0.5 * self.lo + 0.5 * self.hi

    def hw(self):
        with np.errstate(all="ignore"):
            return 0.5 * (self.hi - self.lo)

    def take(self, m):
        return Iv(self.lo[m], self.hi[m])

    def __neg__(self):
        return Iv(-self.hi, -self.lo)

    def __add__(self, o):
        o = _iv(o)
        with np.errstate(all="ignore"):
            return Iv.out(self.lo + o.lo, self.hi + o.hi)

    def __sub__(self, o):
        o = _iv(o)
        with np.errstate(all="ignore"):
            return Iv.out(self.lo - o.hi, self.hi - o.lo)

    def __mul__(self, o):
        o = _iv(o)
        with np.errstate(all="ignore"):
            p = np.stack([self.lo * o.lo, self.lo * o.hi, self.hi * o.lo, self.hi * o.hi])
            bad = np.isnan(p).any(0)
            return Iv.out(np.where(bad, np.nan, p.min(0)), np.where(bad, np.nan, p.max(0)))

    def __truediv__(self, o):
        o = _iv(o)
        with np.errstate(all="ignore"):
            p = np.stack([self.lo / o.lo, self.lo / o.hi, self.hi / o.lo, self.hi / o.hi])
            ok = (o.lo > 0) | (o.hi < 0)
            return Iv.out(np.where(ok, p.min(0), np.nan), np.where(ok, p.max(0), np.nan))

    def __radd__(self, o):
        return _iv(o) + self

    def __rsub__(self, o):
        return _iv(o) - self

    def __rmul__(self, o):
        return _iv(o) * self

    def __rtruediv__(self, o):
        return _iv(o) / self


def _iv(x):
    return x if isinstance(x, Iv) else Iv(x)


def where(m, a, b):
    a, b = _iv(a), _iv(b)
    return Iv(np.where(m, a.lo, b.lo), np.where(m, a.hi, b.hi))


def fma(x, y, z):
    """Color.fma / Float.fma x y z = x y + z: the product interval then the sum interval (covers fused and unfused)."""
    return _iv(x) * y + z


def isqrt(x):
    with np.errstate(all="ignore"):
        return Iv.out(np.sqrt(np.maximum(x.lo, 0.0)), np.sqrt(np.maximum(x.hi, 0.0)))


def iabs(x):
    lo = np.where(x.lo >= 0, x.lo, np.where(x.hi <= 0, -x.hi, 0.0))
    hi = np.maximum(np.abs(x.lo), np.abs(x.hi))
    return Iv(lo, hi)


def imin_const(x, c):  # Base Float.min x c for a constant c (a NaN operand stays NaN)
    return Iv(np.minimum(x.lo, c), np.minimum(x.hi, c))


def iclamp(x, a, b):  # Float.clamp_exn, monotone
    return Iv(np.clip(x.lo, a, b), np.clip(x.hi, a, b))


def _mp_vec(f, *cols):
    """f over mpmath numbers element by element: (lo, hi) binary64 enclosures of the exact values."""
    n = len(cols[0])
    out = np.empty(n)
    for i in range(n):
        args = [_MP.mpf(float(c[i])) if np.isfinite(c[i]) else None for c in cols]
        out[i] = np.nan if any(a is None for a in args) else float(f(*args))
    return _dn(out), _up(out)


def _widen(lo, hi, fn):
    """The measured bound of pt_math.h: |pt_f - f| <= k ulp of f's binade <= k 2^-52 |f|."""
    with np.errstate(all="ignore"):
        w = BOUND_ULPS[fn] * TWO52 * np.maximum(np.abs(lo), np.abs(hi)) * (1 + 2.0 ** -40)
        return Iv(_dn(lo - w), _up(hi + w))


def _unique_eval(f, *cols):
    """Evaluate f on the distinct argument tuples only (endpoints repeat: point inputs, shared hypot arguments)."""
    key = np.stack(cols, axis=1)
    with np.errstate(all="ignore"):
        uniq, inv = np.unique(key, axis=0, return_inverse=True)
    lo, hi = _mp_vec(f, *[uniq[:, k] for k in range(uniq.shape[1])])
    inv = inv.reshape(-1)
    return lo[inv], hi[inv]


def ihypot(x, y):
    ax, ay = iabs(x), iabs(y)
    lo, _ = _unique_eval(_MP.hypot, ax.lo, ay.lo)
    _, hi = _unique_eval(_MP.hypot, ax.hi, ay.hi)
    return _widen(lo, hi, "hypot")


def _trig(x, fn):
    f = _MP.sin if fn == "sin" else _MP.cos
    a_lo, a_hi = _unique_eval(f, x.lo)
    b_lo, b_hi = _unique_eval(f, x.hi)
    lo, hi = np.minimum(a_lo, b_lo), np.maximum(a_hi, b_hi)
    # critical points: sin at pi/2 + k pi, cos at k pi; any one inside (with slack) widens to [-1, 1]
    c0 = 0.5 * PI if fn == "sin" else 0.0
    with np.errstate(all="ignore"):
        k_lo = np.ceil((x.lo - c0) / PI - 1e-9)
        k_hi = np.floor((x.hi - c0) / PI + 1e-9)
        crit = ~(k_lo > k_hi)
    lo, hi = np.where(crit, -1.0, lo), np.where(crit, 1.0, hi)
    return _widen(lo, hi, fn)


def isin(x):
    return _trig(x, "sin")


def icos(x):
    return _trig(x, "cos")


def iacos(x):
    ok = (x.lo >= -1.0) & (x.hi <= 1.0)
    lo, _ = _unique_eval(_MP.acos, np.where(ok, x.hi, 0.0))
    _, hi = _unique_eval(_MP.acos, np.where(ok, x.lo, 0.0))
    r = _widen(lo, hi, "acos")
    return Iv(np.where(ok, r.lo, np.nan), np.where(ok, r.hi, np.nan))


def iatan2(y, x):
    cut = (x.lo <= 0) & (y.lo <= 0) & (y.hi >= 0)  # the branch cut (x < 0, y = 0) or the origin
    los, his = [], []
    for yy in (y.lo, y.hi):
        for xx in (x.lo, x.hi):
            lo, hi = _unique_eval(_MP.atan2, np.where(cut, 1.0, yy), np.where(cut, 1.0, xx))
            los.append(lo)
            his.append(hi)
    r = _widen(np.min(los, axis=0), np.max(his, axis=0), "atan2")
    return Iv(np.where(cut, np.nan, r.lo), np.where(cut, np.nan, r.hi))


def ipow5(x):
    lo, _ = _unique_eval(lambda a: a ** 5, x.lo)
    _, hi = _unique_eval(lambda a: a ** 5, x.hi)
    return _widen(lo, hi, "pow5")


# ---------------------------------------------------------------- decisions
class Decisions:
    """Per sample: robust (every decision so far robust) and the closeness |mid - b| / half-width of named ones."""

    def __init__(self, n):
        self.robust = np.ones(n, bool)
        self.ratio = {}

    def decide(self, name, q, boundary, active=None):
        """Returns q > boundary at the midpoint; marks inactive-or-robust samples.  Non-finite intervals fail."""
        m, h = q.mid(), q.hw()
        with np.errstate(all="ignore"):
            gap = np.abs(m - boundary)
            ok = np.isfinite(m) & np.isfinite(h) & (gap > MARGIN * h)
            r = np.where(h > 0, gap / h, np.where(gap > 0, np.inf, 0.0))
        if active is None:
            active = np.ones(len(m), bool)
        self.robust &= ok | ~active
        prev = self.ratio.get(name)
        r = np.where(active, r, np.inf)
        self.ratio[name] = r if prev is None else np.minimum(prev, r)
        return m > boundary

    def require_finite(self, *ivs, active=None):
        ok = np.ones(len(self.robust), bool)
        for v in ivs:
            ok &= np.isfinite(v.lo) & np.isfinite(v.hi)
        self.robust &= ok | (~active if active is not None else False)


# ---------------------------------------------------------------- vectors and quaternions of intervals
def V(x, y, z):
    return (_iv(x), _iv(y), _iv(z))


def vadd(a, b):
    return tuple(a[k] + b[k] for k in range(3))


def vsub(a, b):
    return tuple(a[k] - b[k] for k in range(3))


def vmul(a, b):
    return tuple(a[k] * b[k] for k in range(3))


def vscale(a, s):  # V3.scale v s = map (( *. ) s)
    return tuple(_iv(s) * a[k] for k in range(3))


def vneg(a):
    return tuple(-a[k] for k in range(3))


def vfma(u, v, w):
    return tuple(fma(u[k], v[k], w[k]) for k in range(3))


def vdot(a, b):
    return fma(a[0], b[0], fma(a[1], b[1], a[2] * b[2]))


def vcross(p, q):
    def h(w, x, y, z):
        return fma(w, x, -(y * z))
    a, b, c = p
    d, e, f = q
    return (h(b, f, c, e), h(c, d, a, f), h(a, e, b, d))


def vnormalize(v):
    return vscale(v, 1.0 / ihypot(v[0], ihypot(v[1], v[2])))


def vwhere(m, a, b):
    return tuple(where(m, a[k], b[k]) for k in range(3))


def vtake(a, m):
    return tuple(a[k].take(m) for k in range(3))


def qnormalize(r, v):
    s = 1.0 / ihypot(ihypot(r, v[0]), ihypot(v[1], v[2]))
    return r * s, vscale(v, s)


def qmul(a, b):
    ar, av = a
    br, bv = b
    r = ar * br - vdot(av, bv)
    v = vadd(vadd(vcross(av, bv), vscale(bv, ar)), vscale(av, br))
    return r, v


def qconj(q):
    return q[0], vneg(q[1])


def qtransform(q, v):
    zero = Iv(np.zeros_like(v[0].lo))
    return qmul(qmul(q, (zero, v)), qconj(q))[1]


# ---------------------------------------------------------------- scene tables
class Tables:
    """What shading reads from a ptx_scene_desc: materials, textures, per-primitive tex coords and materials, camera,
    background, plus the exact_geometry.Geometry of the build list and the floor."""

    def __init__(self, desc_ptr):
        d = desc_ptr.contents if hasattr(desc_ptr, "contents") else desc_ptr
        self.geo = X.Geometry(d)
        g = self.geo
        M = [d.materials[i] for i in range(d.n_materials)]
        self.m_kind = np.array([m.kind for m in M], np.int32)
        self.m_tex = np.array([m.texture for m in M], np.int32)
        self.m_index = np.array([m.index for m in M])
        self.m_emit = np.array([list(m.emit) for m in M]).reshape(-1, 3)
        T = [d.textures[i] for i in range(d.n_textures)]
        self.t_kind = np.array([t.kind for t in T], np.int32)
        self.t_w = np.array([t.width for t in T], np.int64)
        self.t_h = np.array([t.height for t in T], np.int64)
        self.t_even = np.array([list(t.even) for t in T]).reshape(-1, 3)
        self.t_odd = np.array([list(t.odd) for t in T]).reshape(-1, 3)
        nt, ns, nf = g.n_tri, g.n_sph, g.n_floor
        uv = [np.ctypeslib.as_array(d.tri_uv, shape=(6 * nt,)).reshape(nt, 6)] if nt else []
        mat = [np.ctypeslib.as_array(d.tri_material, shape=(nt,))] if nt else []
        uv.append(np.zeros((ns, 6)))
        mat.append(np.ctypeslib.as_array(d.sphere_material, shape=(ns,)) if ns else np.zeros(0, np.int32))
        if nf:
            uv.append(np.ctypeslib.as_array(d.floor_uv, shape=(6 * nf,)).reshape(nf, 6))
            mat.append(np.ctypeslib.as_array(d.floor_material, shape=(nf,)))
        self.uv = np.concatenate(uv).copy()
        self.mat = np.concatenate(mat).astype(np.int32)
        c = d.camera
        self.cam4 = np.array([c.lower_left_x, c.lower_left_y, c.view_x, c.view_y])
        self.bg_kind = d.background.kind
        self.horizon = np.array(list(d.background.horizon))
        self.zenith = np.array(list(d.background.zenith))

    def is_sphere(self, prim):
        return (prim >= self.geo.n_tri) & (prim < self.geo.n_prims)


# ---------------------------------------------------------------- sampler and camera
def lds_alpha(oracle, dim):
    a = np.zeros(dim)
    oracle.lib().orc_lds_alpha(dim, oracle._dp(a))
    return a


def sampler(alpha, offsets, dim, dec, name="sampler"):
    """L.get alpha offset dim = frac(0.5 + alpha_dim (1 + offset)): (binary64 value, interval).  The trunc is a
    decision (the value jumps at every integer)."""
    a = Iv(np.full(len(offsets), alpha[dim]))
    x = 0.5 + a * Iv((1 + offsets).astype(np.float64))
    dec.decide(name, _frac_q(x), 0.0)
    t = np.trunc(x.mid())
    val = x - Iv(t)
    with np.errstate(all="ignore"):
        point = 0.5 + alpha[dim] * (1 + offsets).astype(np.float64)
    return point - np.trunc(point), val


def _frac_q(x):
    """x - nearest integer (an interval): its sign change marks an integer inside x."""
    k = np.round(x.mid())
    return Iv(x.lo - k, x.hi - k)  # exact: Sterbenz for |x - k| <= 1/2 and k, x of like magnitude (x < 2^52)


def camera_samples(tab, alpha, width, height, spp, xs, ys, ps, dec):
    """cx, cy (binary64 values, what render_tile forms) and the restated camera direction interval."""
    off = ys.astype(np.int64) * width + xs + ps.astype(np.int64) * spp
    dx, dx_iv = sampler(alpha, off, 0, dec)
    dy, dy_iv = sampler(alpha, off, 1, dec)
    wf, hf = 1.0 / width, 1.0 / height
    cx = (xs.astype(np.float64) + dx) * wf
    cy = 1.0 - ((ys.astype(np.float64) + dy) * hf)
    cx_iv = (Iv(xs.astype(np.float64)) + dx_iv) * wf
    cy_iv = 1.0 - ((Iv(ys.astype(np.float64)) + dy_iv) * hf)
    llx, lly, vx, vy = tab.cam4
    n = len(xs)
    d = vnormalize(V(llx + Iv(np.full(n, vx)) * cx_iv, lly + Iv(np.full(n, vy)) * cy_iv, Iv(np.full(n, -1.0))))
    return cx, cy, d


def oracle_camera_rays(oracle, cam4, cx, cy):
    """The binary64 camera ray of each sample through orc_camera_ray (an input of the restatement, checked against
    the restated camera by the caller)."""
    out = np.zeros(6)
    D = np.zeros((len(cx), 3))
    c4 = np.ascontiguousarray(cam4, dtype=np.float64)
    for i in range(len(cx)):
        oracle.lib().orc_camera_ray(oracle._dp(c4), float(cx[i]), float(cy[i]), oracle._dp(out))
        assert out[0] == 0.0 and out[1] == 0.0 and out[2] == 0.0
        D[i] = out[3:]
    return D


def inside(iv3, got):
    """Per sample: every component of got (n, k) lies in its interval."""
    ok = np.ones(got.shape[0], bool)
    for k, iv in enumerate(iv3):
        ok &= (iv.lo <= got[:, k]) & (got[:, k] <= iv.hi)
    return ok


def rel_width(iv3, floor=0.0):
    """Largest component width over the norm of the midpoint vector (at least `floor`)."""
    w = np.max([iv.hi - iv.lo for iv in iv3], axis=0)
    n = np.maximum(np.sqrt(sum(iv.mid() ** 2 for iv in iv3)), floor)
    with np.errstate(all="ignore"):
        return np.where(n > 0, w / n, np.where(w == 0, 0.0, np.inf))


# ---------------------------------------------------------------- one segment: hit, shading, scatter
def _fr_iv(q, e):
    """[q - e, q + e] rounded outward, q a Fraction (or float), e a float bound."""
    f = np.array([float(x) for x in q])
    e = np.asarray(e, dtype=np.float64)
    with np.errstate(all="ignore"):
        return Iv(_dn(_dn(f) - e), _up(_up(f) + e))


def hit_params(tab, res, O, D):
    """The exact hit parameters of every robust hit: t (spheres) and u, v (triangles, floor) as intervals."""
    g = tab.geo
    n = len(O)
    hit = res.robust & (res.prim >= 0)
    t_iv = Iv(np.full(n, np.nan))
    u_iv, v_iv = Iv(np.full(n, np.nan)), Iv(np.full(n, np.nan))
    sph = hit & tab.is_sphere(res.prim)
    if sph.any():
        t = res.t_exact[sph]
        t_iv.lo = t_iv.lo.copy()
        t_iv.hi = t_iv.hi.copy()
        iv = _fr_iv(t, res.t_bound[sph])
        t_iv.lo[sph], t_iv.hi[sph] = iv.lo, iv.hi
    tri = hit & ~tab.is_sphere(res.prim)
    if tri.any():
        idx = np.nonzero(tri)[0]
        p = res.prim[idx]
        fl = p >= g.n_prims
        A = np.where(fl[:, None], g.floor_a[np.clip(p - g.n_prims, 0, max(g.n_floor - 1, 0))] if g.n_floor else 0.0,
                     g.tri_a[np.clip(p, 0, max(g.n_tri - 1, 0))] if g.n_tri else 0.0)
        B = np.where(fl[:, None], g.floor_b[np.clip(p - g.n_prims, 0, max(g.n_floor - 1, 0))] if g.n_floor else 0.0,
                     g.tri_b[np.clip(p, 0, max(g.n_tri - 1, 0))] if g.n_tri else 0.0)
        Cc = np.where(fl[:, None], g.floor_c[np.clip(p - g.n_prims, 0, max(g.n_floor - 1, 0))] if g.n_floor else 0.0,
                      g.tri_c[np.clip(p, 0, max(g.n_tri - 1, 0))] if g.n_tri else 0.0)
        ev = X.tri_prepass(A, B, Cc, O[idx], D[idx])
        us, vs = [], []
        for k, i in enumerate(idx):
            ex = X.tri_exact(A[k], B[k], Cc[k], O[i], D[i])
            us.append(ex["u"])
            vs.append(ex["v"])
        ui, vi = _fr_iv(us, ev["u"].e), _fr_iv(vs, ev["v"].e)
        u_iv = Iv(u_iv.lo.copy(), u_iv.hi.copy())
        v_iv = Iv(v_iv.lo.copy(), v_iv.hi.copy())
        u_iv.lo[idx], u_iv.hi[idx], v_iv.lo[idx], v_iv.hi[idx] = ui.lo, ui.hi, vi.lo, vi.hi
    return hit, sph, tri, t_iv, u_iv, v_iv


def _prim_vertices(tab, prim):
    g = tab.geo
    out = []
    for which in ("a", "b", "c"):
        tri = getattr(g, "tri_" + which)
        flo = getattr(g, "floor_" + which)
        allv = np.concatenate([tri, np.zeros((g.n_sph, 3)), flo]) if len(tri) + g.n_sph + len(flo) else np.zeros((1, 3))
        out.append(allv[np.clip(prim, 0, len(allv) - 1)])
    return out


def shader_space(normal, dec, mut, active):
    """Shader_space.create: the rotation quaternion, both pole tests being decisions."""
    eps = 1e-8 if "pole_eps_1e-8" in mut else 1e-9
    eps_bot = 1e-8 if "pole_bottom_eps_1e-8" in mut else eps
    z = normal[2]
    top = dec.decide("pole_top", z, 1.0 - eps, active)
    bot = ~dec.decide("pole_bottom", z, eps_bot - 1.0, active)
    n = len(z.lo)
    one, zero = Iv(np.ones(n)), Iv(np.zeros(n))
    r, v = qnormalize(1.0 + z, V(normal[1], -normal[0], zero))
    r = where(top, one, where(bot, zero, r))
    v = vwhere(top, V(zero, zero, zero), vwhere(bot, V(zero, one, zero), v))
    return r, v


def rotate(q, v):
    return qtransform(q, v)


def rotate_inv(q, v, mut=()):
    return qtransform(q if "rotate_not_inv" in mut else qconj(q), v)


def world_ray(q, origin, dir_ss, mut):
    d = rotate_inv(q, dir_ss, mut)
    off = 1e-4 if "offset_1e-4" in mut else 1e-3
    return vadd(origin, vscale(d, off)), d


def hemisphere(u, v, mut):
    r = isqrt(u)
    theta = (v * 2.0) * PI
    x, y = r * icos(theta), r * isin(theta)
    z = isqrt(1.0 - u)
    return (y, x, z) if "hemisphere_xy_swapped" in mut else (x, y, z)


def texture(tab, tex, tu, tv, dec, mut, active):
    """Texture.eval: (n, 3) colours, with the checker's parity decisions."""
    tex = np.clip(tex, 0, len(tab.t_kind) - 1)
    checker = active & (tab.t_kind[tex] == 1)
    dw = 0 if "checker_width_not_minus_1" in mut else 1
    w = Iv((tab.t_w[tex] - dw).astype(np.float64))
    h = Iv((tab.t_h[tex] - dw).astype(np.float64))
    xp, yp = tu * w, tv * h
    dec.decide("checker", _frac_q(xp), 0.0, checker)
    dec.decide("checker", _frac_q(yp), 0.0, checker)
    dec.require_finite(xp, yp, active=checker)
    with np.errstate(all="ignore"):
        px = np.nan_to_num(np.trunc(xp.mid())).astype(np.int64) & 1
        py = np.nan_to_num(np.trunc(yp.mid())).astype(np.int64) & 1
    even = (px == py) if "checker_swapped" not in mut else (px != py)
    even = even | (tab.t_kind[tex] == 0)
    return np.where(even[:, None], tab.t_even[tex], tab.t_odd[tex])


def _pt(a):
    return Iv(np.asarray(a, dtype=np.float64))


def segment(tab, O, D, res, u, v, dec, mut=()):
    """One segment from the point rays (O, D) whose closest hits are `res` (exact_geometry.Result), with the sampler
    values u, v (intervals) of this bounce.  Returns a dict of arrays and intervals; dec collects the decisions."""
    n = len(O)
    dec.robust &= res.robust
    hit, sph, tri, t_iv, u_iv, v_iv = hit_params(tab, res, O, D)
    prim = np.where(hit, res.prim, 0)
    o3, d3 = V(*[_pt(O[:, k]) for k in range(3)]), V(*[_pt(D[:, k]) for k in range(3)])
    # ---- sphere hits (sphere.ml:21-33, 56-69)
    g = tab.geo
    cen = np.concatenate([np.zeros((g.n_tri, 3)), g.sph_c, np.zeros((g.n_floor, 3))])[np.clip(prim, 0, g.n_prims + g.n_floor - 1)] \
        if g.n_prims + g.n_floor else np.zeros((n, 3))
    ps = vadd(o3, vscale(d3, t_iv))
    ns = vnormalize(vsub(ps, V(*[_pt(cen[:, k]) for k in range(3)])))
    # ---- triangle hits (triangle.ml:24-64)
    A, B, Cc = _prim_vertices(tab, prim)
    a3, b3, c3 = (V(*[_pt(P[:, k]) for k in range(3)]) for P in (A, B, Cc))
    gn = vnormalize(vcross(vsub(b3, a3), vsub(c3, a3)))
    w = (1.0 - u_iv) - v_iv
    pt = vadd(vadd(vscale(a3, w), vscale(b3, u_iv)), vscale(c3, v_iv))
    uv = tab.uv[prim]
    tu_t = (_pt(uv[:, 0]) * w + _pt(uv[:, 2]) * u_iv) + _pt(uv[:, 4]) * v_iv  # w2 = 1 - u - v again: the same value
    tv_t = (_pt(uv[:, 1]) * w + _pt(uv[:, 3]) * u_iv) + _pt(uv[:, 5]) * v_iv
    # ---- hit_front and the shading normal
    n0 = vwhere(sph, ns, gn)
    point = vwhere(sph, ps, pt)
    front = ~dec.decide("hit_front", vdot(d3, n0), 0.0, hit)
    normal = vwhere(front, n0, vneg(n0))
    theta = iacos(-normal[1])
    phi = PI + iatan2(-normal[2], normal[0])
    one_over_pi, one_over_two_pi = 1.0 / PI, 1.0 / (2.0 * PI)
    tu = where(sph, phi * one_over_two_pi, tu_t)
    tv = where(sph, theta * one_over_pi, tv_t)
    q = shader_space(normal, dec, mut, hit)
    omega_i = rotate(q, vneg(d3))
    mat = tab.mat[prim]
    kind_m = np.where(hit, tab.m_kind[mat], -1)
    emit = np.where(hit[:, None], tab.m_emit[mat], 0.0)
    lam, met, die = hit & (kind_m == MAT_LAMBERTIAN), hit & (kind_m == MAT_METAL), hit & (kind_m == MAT_DIELECTRIC)
    col = texture(tab, tab.m_tex[mat], tu, tv, dec, mut, lam | met)
    dec.require_finite(tu, tv, active=(lam | met) & (tab.t_kind[np.clip(tab.m_tex[mat], 0, len(tab.t_kind) - 1)] == 1))
    # ---- Metal
    omega_r = (-omega_i[0], -omega_i[1], omega_i[2])
    m_absorb = ~dec.decide("metal_z", omega_r[2], 0.0, met)
    col3 = V(*[_pt(col[:, k]) for k in range(3)])
    sp = ipow5(1.0 - omega_i[2])
    m_att = vadd(col3, vscale(vsub(V(1.0, 1.0, 1.0), col3), sp))
    m_o, m_d = world_ray(q, point, omega_r, mut)
    # ---- Dielectric
    index = _pt(tab.m_index[mat])
    index_inv = 1.0 / index
    c = iclamp(omega_i[2], 0.0, 1.0)
    s = isqrt(1.0 - c * c)
    use_inv = ~front if "index_swapped" in mut else front
    ratio = where(use_inv, index_inv, index)
    tir = dec.decide("tir", ratio * s, 1.0, die)
    qq = (1.0 - ratio) / (1.0 + ratio)
    r0 = qq * qq
    schlick = r0 + (1.0 - r0) * ipow5(1.0 - c)
    refl = dec.decide("schlick", schlick - u, 0.0, die & ~tir) | tir
    cc = imin_const(omega_i[2], 1.0)
    perp = vscale(vsub(V(0.0, 0.0, cc), omega_i), ratio)
    para_z = -isqrt(iabs(1.0 - vdot(perp, perp)))
    refr = (perp[0] + 0.0, perp[1] + 0.0, perp[2] + para_z)
    wo = vwhere(refl, omega_r, refr)
    g_o, g_d = world_ray(q, point, wo, mut)
    # ---- Lambertian: the diffuse branch of the path loop
    h = hemisphere(u, v, mut)
    pd_zero = ~dec.decide("pd", h[2], 0.0, lam)
    l_o, l_d = world_ray(q, point, h, mut)
    # ---- assemble
    kind = np.full(n, -1)
    kind[lam] = SC_DIFFUSE
    kind[met] = np.where(m_absorb[met], SC_ABSORB, SC_SPECULAR)
    kind[die] = SC_SPECULAR
    alive = (kind == SC_SPECULAR) | ((kind == SC_DIFFUSE) & ~pd_zero)
    ray_o = vwhere(met, m_o, vwhere(die, g_o, l_o))
    ray_d = vwhere(met, m_d, vwhere(die, g_d, l_d))
    att = vwhere(met, m_att, vwhere(die, V(1.0, 1.0, 1.0), col3))
    dec.require_finite(*ray_o, *ray_d, *att, active=alive)
    return {"hit": hit, "prim": np.where(hit, res.prim, -1), "mat_kind": kind_m, "kind": kind, "alive": alive,
            "ray_o": ray_o, "ray_d": ray_d, "att": att, "emit": emit, "dir": d3}


def background(tab, d3):
    n = len(d3[0].lo)
    if tab.bg_kind == 0:
        return V(np.zeros(n), np.zeros(n), np.zeros(n))
    d = vnormalize(d3)
    z = Iv(np.zeros(n))
    t = 0.5 * (vdot(d, V(z, Iv(np.ones(n)), z)) + 1.0)
    hz = V(*[Iv(np.full(n, tab.horizon[k])) for k in range(3)])
    zn = V(*[Iv(np.full(n, tab.zenith[k])) for k in range(3)])
    return vadd(vscale(hz, 1.0 - t), vscale(zn, t))


def accumulate(emit0, attn0, emit, att, mut):
    """A scatter in the path loop: emit0 <- add_mul emit att emit0 = fma(att, emit0, emit); attn0 <- att attn0."""
    ne = vfma(attn0, emit, emit0) if "add_mul_physical" in mut else vfma(att, emit0, emit)
    return ne, vmul(att, attn0)


# ---------------------------------------------------------------- a sample set through the restatement
class Samples:
    """Samples (x, y, pass) of one scene at one max_bounces: the camera rays (binary64, checked against the restated
    camera), the exact closest hits of the first segment and the sampler values of the first two bounces."""

    def __init__(self, oracle, tab, width, height, spp, max_bounces, xs, ys, ps):
        self.tab, self.width, self.height, self.spp, self.mb = tab, width, height, spp, max_bounces
        self.xs, self.ys, self.ps = (np.ascontiguousarray(a, dtype=np.int32) for a in (xs, ys, ps))
        n = len(self.xs)
        self.alpha = lds_alpha(oracle, 2 + 2 * max_bounces)
        self.dec0 = Decisions(n)
        cx, cy, self.d_iv = camera_samples(tab, self.alpha, width, height, spp, self.xs, self.ys, self.ps, self.dec0)
        self.D = oracle_camera_rays(oracle, tab.cam4, cx, cy)
        self.camera_ok = inside(self.d_iv, self.D)
        self.O = np.zeros_like(self.D)
        self.ref = X.Reference(tab.geo)
        self.res = self.ref.closest(self.O, self.D)
        off = self.ys.astype(np.int64) * width + self.xs + self.ps.astype(np.int64) * spp
        self.uv = []
        for j in range(max_bounces):
            u = sampler(self.alpha, off, 2 + 2 * j, self.dec0)[1]
            v = sampler(self.alpha, off, 3 + 2 * j, self.dec0)[1]
            self.uv.append((u, v))

    def first(self, mut=()):
        """The first segment: Decisions and the segment dict."""
        dec = Decisions(len(self.xs))
        dec.robust &= self.dec0.robust
        u, v = self.uv[0] if self.uv else (Iv(np.full(len(self.xs), 0.5)), Iv(np.full(len(self.xs), 0.5)))
        return dec, segment(self.tab, self.O, self.D, self.res, u, v, dec, mut)

    def radiance(self, next_o=None, next_d=None, mut=()):
        """The radiance of every sample at self.mb (0, 1 or 2) as an interval and its Decisions.  For 2 the second
        segment starts from the binary64 next ray (next_o, next_d) the caller has checked against the enclosure of the
        first scatter; its closest hit is exact_geometry's."""
        n = len(self.xs)
        zero = V(np.zeros(n), np.zeros(n), np.zeros(n))
        ones = V(np.ones(n), np.ones(n), np.ones(n))
        if self.mb == 0:
            dec = Decisions(n)
            return dec, vfma(ones, zero, zero)
        dec, s1 = self.first(mut)
        em1 = V(*[_pt(s1["emit"][:, k]) for k in range(3)])
        miss1 = vfma(ones, background(self.tab, s1["dir"]), zero)
        absorb1 = vfma(ones, em1, zero)
        e1, a1 = accumulate(zero, ones, em1, s1["att"], mut)
        out = vwhere(~s1["hit"], miss1, vwhere(~s1["alive"], absorb1, vfma(a1, zero, e1)))
        if self.mb == 1:
            return dec, out
        live = s1["alive"]
        O2 = np.where(live[:, None], next_o, 0.0)
        D2 = np.where(live[:, None], next_d, np.array([0.0, 0.0, -1.0]))
        res2 = self.ref.closest(O2, D2)
        dec2 = Decisions(n)
        s2 = segment(self.tab, O2, D2, res2, self.uv[1][0], self.uv[1][1], dec2, mut)
        dec.robust &= dec2.robust | ~live
        for k, r in dec2.ratio.items():
            dec.ratio[k + "_2"] = np.where(live, r, np.inf)
        em2 = V(*[_pt(s2["emit"][:, k]) for k in range(3)])
        miss2 = vfma(a1, background(self.tab, s2["dir"]), e1)
        absorb2 = vfma(a1, em2, e1)
        e2, a2 = accumulate(e1, a1, em2, s2["att"], mut)
        cont2 = vfma(a2, zero, e2)
        two = vwhere(~s2["hit"], miss2, vwhere(~s2["alive"], absorb2, cont2))
        return dec, vwhere(live, two, out)


# ---------------------------------------------------------------- comparisons
def check_first_scatter(smp, ray, att, alive, info=None, mut=()):
    """Messages (empty when the robust samples agree) and a summary dict.  ray (n, 6), att (n, 3), alive (n,),
    info (n, 3) = prim, material kind, scatter kind (orc_debug_first_scatter's info_out) or None."""
    dec, s = smp.first(mut)
    rob = dec.robust & smp.camera_ok
    bad = []
    n = len(alive)
    if info is not None:
        hit = s["hit"]
        for name, got, want, m in (("prim", info[:, 0], s["prim"], rob),
                                   ("material kind", info[:, 1], s["mat_kind"], rob & hit),
                                   ("scatter kind", info[:, 2], s["kind"], rob & hit)):
            w = np.nonzero(m & (got != want))[0]
            if len(w):
                bad.append(f"{len(w)} robust samples: {name} {int(got[w[0]])} != restated {int(want[w[0]])} (sample {w[0]})")
    a = alive.astype(bool)
    w = np.nonzero(rob & (a != s["alive"]))[0]
    if len(w):
        bad.append(f"{len(w)} robust samples: alive {int(a[w[0]])} != restated {int(s['alive'][w[0]])} (sample {w[0]})")
    live = rob & s["alive"] & a
    for name, iv3, got in (("origin", s["ray_o"], ray[:, :3]), ("direction", s["ray_d"], ray[:, 3:]), ("attenuation", s["att"], att)):
        ok = inside(iv3, got)
        w = np.nonzero(live & ~ok)[0]
        if len(w):
            k = w[0]
            bad.append(f"{len(w)} robust samples: {name} outside its enclosure, e.g. sample {k}: {got[k].tolist()} not in "
                       f"{[(iv.lo[k], iv.hi[k]) for iv in iv3]}")
    summ = {"samples": n, "robust": int(rob.sum()), "alive": int(live.sum()),
            "camera_outside": int((~smp.camera_ok).sum())}
    for name, iv3 in (("dir", s["ray_d"]), ("origin", s["ray_o"]), ("att", s["att"])):
        summ[f"p99_rel_width_{name}"] = float(np.percentile(rel_width(vtake(iv3, live)), 99)) if live.any() else 0.0
    return bad, summ, dec, s


def check_radiance(smp, rgb, next_o=None, next_d=None, mut=(), target=None):
    """Messages, a summary dict (with near_<target>: robust samples within 100 half-widths of that decision) and the
    robust mask of the radiance comparison."""
    dec, iv3 = smp.radiance(next_o, next_d, mut)
    rob = dec.robust & smp.camera_ok
    ok = inside(iv3, rgb)
    w = np.nonzero(rob & ~ok)[0]
    bad = []
    if len(w):
        k = w[0]
        bad.append(f"{len(w)} robust samples: radiance outside its enclosure, e.g. sample {k}: {rgb[k].tolist()} not in "
                   f"{[(iv.lo[k], iv.hi[k]) for iv in iv3]}")
    rw = rel_width(vtake(iv3, rob), floor=1e-3)  # a black radiance has no relative width: colours below 1e-3 count as 1e-3
    summ = {"samples": len(rgb), "robust": int(rob.sum()),
            "p99_rel_width_radiance": float(np.percentile(rw[np.isfinite(rw)], 99)) if rob.any() else 0.0}
    if target is not None:
        summ["near_" + target] = near_count(dec, target, rob)
    return bad, summ, rob


MAX_REL_WIDTH = 1e-10
MIN_ROBUST, MIN_NEAR = 0.50, 0.20


# Three families sit where the binary64 computation itself is ill-conditioned, so a tight enclosure is impossible there:
# a refraction just short of TIR takes sqrt(1 - |perp|^2) of a quantity near 0 (its derivative is unbounded); a ray
# that grazes a sphere fixes t, hence the hit point and the normal, only to ~u / omega_i.z; and just off the bottom pole
# Shader_space.create builds its rotation from 1 + z ~ 1e-9 and normal x, y ~ 4.5e-5, known to ~1e-7 and ~1e-12
# relative.  Their bound is ~10x the largest 99th-percentile width measured there (tir 1.0e-7, metal_grazing 9.5e-6,
# pole_bottom 3.2e-10, its radiance); every other scene and family is held to MAX_REL_WIDTH.
ILL_CONDITIONED = {"tir": 1e-6, "metal_grazing": 1e-4, "pole_bottom": 3e-9}


def check_tightness(name, summ):
    lim = ILL_CONDITIONED.get(name, MAX_REL_WIDTH)
    return [f"{name}: 99th-percentile relative width of the {k[len('p99_rel_width_'):]} enclosure {v:.3e} > {lim}"
            for k, v in summ.items() if k.startswith("p99_rel_width_") and not v <= lim]


def near_count(dec, target, rob):
    r = dec.ratio.get(target)
    return 0 if r is None else int((rob & (r <= 100)).sum())


# ---------------------------------------------------------------- scenes: stock, soups, and families aimed at boundaries
def make_scene_desc(abi, spheres=(), tris=(), tri_uv=None, materials=None, textures=None, background=None, leaf_kind=1,
                    cutoff=4):
    """exact_geometry.make_desc with per-triangle tex coords, a material table, a texture table and a background."""
    return X.make_desc(abi, spheres=spheres, tris=tris, leaf_kind=leaf_kind, cutoff=cutoff, tri_uv=tri_uv,
                       materials=materials, textures=textures, background=background)


def shading_soup(seed, n=160):
    """Spheres and triangles in front of the camera, with every material on both primitive kinds: solid and checker
    textures, metals, dielectrics of two indices, emitters, and triangles facing either way."""
    rng = np.random.default_rng(seed)
    textures = [(0, 1, 1, (0.8, 0.5, 0.3), (0, 0, 0)), (1, 8, 16, (0.9, 0.9, 0.9), (0.1, 0.2, 0.3)),
                (1, 101, 57, (0.2, 0.7, 0.4), (0.6, 0.1, 0.9)), (0, 1, 1, (0.95, 0.9, 0.7), (0, 0, 0))]
    materials = [(MAT_LAMBERTIAN, 0, 0.0, (0, 0, 0)), (MAT_LAMBERTIAN, 1, 0.0, (0, 0, 0)), (MAT_METAL, 3, 0.0, (0, 0, 0)),
                 (MAT_METAL, 2, 0.0, (0, 0, 0)), (MAT_DIELECTRIC, 0, 1.5, (0, 0, 0)), (MAT_DIELECTRIC, 0, 2.4, (0, 0, 0)),
                 (MAT_LAMBERTIAN, 2, 0.0, (3.0, 2.0, 1.0)), (MAT_METAL, 1, 0.0, (0.5, 0.5, 0.5))]
    sphs, tris, uvs = [], [], []
    for _ in range(n):
        z = -rng.uniform(2.0, 12.0)
        c = np.array([rng.uniform(-1.0, 1.0) * -z, rng.uniform(-0.5, 0.5) * -z, z])
        size = rng.uniform(0.05, 0.6) * -z / 8
        m = int(rng.integers(0, len(materials)))
        if rng.random() < 0.5:
            sphs.append((*c, size, m))
        else:
            p = c + rng.normal(size=(3, 3)) * size
            tris.append((p[0], p[1], p[2], m))
            uvs.append(rng.uniform(-0.2, 1.2, 6))
    return sphs, tris, np.array(uvs).reshape(-1), materials, textures


def stock_desc(name, oracle, abi):
    """(desc pointer, keepalive, width, height, spp)."""
    if name.startswith("shade_soup"):
        seed = int(name.split("-")[1])
        sphs, tris, uv, mats, texs = shading_soup(seed)
        bg = "black" if seed % 2 else "sky"
        d, keep = make_scene_desc(abi, sphs, tris, uv, mats, texs, bg)
        return C.pointer(d), (d, keep), 96, 48, 4
    W, H = {"shirley": (120, 60), "shirley_no_simd": (120, 60), "cornell": (64, 64), "ganesha_3k": (64, 36),
            "ganesha_150k": (64, 36)}[name]
    ptr, keep = X.scene_desc(name, oracle, abi)
    return ptr, keep, W, H, 4


STOCK = ["shirley", "shirley_no_simd", "cornell", "ganesha_3k", "shade_soup-1", "shade_soup-2", "shade_soup-3"]


def random_samples(name, W, H, spp, n=3000):
    rng = np.random.default_rng(sum(map(ord, name)) + 17)
    return rng.integers(0, W, n), rng.integers(0, H, n), rng.integers(0, spp, n)


# families: name -> target decision.  Each places one small primitive on the camera ray of every sample of a grid of
# pixels (every other pixel and row of a 2G x 2G image, pass 0, spp 1), sized well below the spacing of neighbouring
# sampled rays at its depth, and solved in mpmath so that the target quantity sits at its boundary; rounding the
# primitive to binary64 leaves samples on both sides and some undecided.  The sampler's alpha depends on the number of
# dimensions, 2 + 2 max_bounces, so the camera rays the primitives are solved on are those of max_bounces FAMILY_MB
# only; the families are run at that depth alone.
#
# What the families can and cannot reach:
# * camera rays travel towards -z, so a first hit only meets the top pole test (z > 1 - 1e-9); "pole" faces the
#   camera and away from it (the shading normal is then -g) to reach it both ways.  The bottom pole test
#   (z < 1e-9 - 1) needs a second segment: "pole_bottom" (target "pole_bottom_2", the second hit's decision).
# * metal's absorb rule: for a hit from outside omega_r.z = omega_i.z > 0 exactly, so its absorb side is never
#   robust; "metal_grazing" pins the scatter side down to omega_i.z ~ 2.5e-6 (a wrong threshold below that passes).
FAMILY_GRID = 31  # 961 primitives: the per-slot frame table (<= 1024 slots) is in use
FAMILY_MB = 2
FAMILIES = {"pole": "pole_top", "pole_bottom": "pole_bottom_2", "checker_tri": "checker", "checker_sph": "checker",
            "tir": "tir", "schlick": "schlick", "metal_grazing": "metal_z", "emit_sky": "checker", "emit_black": "checker"}


def family_samples(name):
    """Every other pixel of a 62 x 62 image; pole_bottom (two primitives per sample, the second off to the side of the
    camera ray) every fourth pixel of a 64 x 64 image, so that its second triangle lies between sampled columns."""
    grid, stride = (16, 4) if name == "pole_bottom" else (FAMILY_GRID, 2)
    j, i = np.meshgrid(np.arange(grid), np.arange(grid), indexing="ij")
    return (stride * i).reshape(-1), (stride * j).reshape(-1), np.zeros(grid * grid, np.int64), stride * grid, stride * grid, 1


def _camera_of(abi):
    d, _ = X.make_desc(abi)
    c = d.camera
    return np.array([c.lower_left_x, c.lower_left_y, c.view_x, c.view_y])


def _basis(n):
    """Two unit vectors completing n (unit, mpmath) to a right-handed frame (e1 x e2 = n)."""
    a = [_MP.mpf(1), _MP.mpf(0), _MP.mpf(0)] if abs(n[0]) < 0.6 else [_MP.mpf(0), _MP.mpf(1), _MP.mpf(0)]
    e1 = _mcross(a, n)
    e1 = _mnorm(e1)
    e2 = _mcross(n, e1)
    return e1, e2


def _mcross(p, q):
    return [p[1] * q[2] - p[2] * q[1], p[2] * q[0] - p[0] * q[2], p[0] * q[1] - p[1] * q[0]]


def _mnorm(v):
    s = _MP.sqrt(sum(x * x for x in v))
    return [x / s for x in v]


def _tri_around(P, n, rho, rot):
    """A triangle of circumradius rho centred at P in the plane of unit normal n, wound so that
    cross(b - a, c - a) points along n; rounded to binary64."""
    e1, e2 = _basis(n)
    pts = []
    for k in range(3):
        ang = rot + 2 * _MP.pi * k / 3
        pts.append(tuple(float(P[i] + rho * (_MP.cos(ang) * e1[i] + _MP.sin(ang) * e2[i])) for i in range(3)))
    return pts


def _offset(rng, lo, hi):
    """A signed offset of log-uniform magnitude in [lo, hi]: a few to a hundred half-widths of the target quantity."""
    return _MP.mpf(float(rng.choice([-1.0, 1.0]) * 10.0 ** rng.uniform(np.log10(lo), np.log10(hi))))


def family_desc(name, oracle, abi):
    """(desc pointer, keepalive, width, height, spp, xs, ys, ps) of a designed family."""
    xs, ys, ps, W, H, spp = family_samples(name)
    rng = np.random.default_rng(sum(map(ord, name)))
    cam4 = _camera_of(abi)
    alpha = lds_alpha(oracle, 2 + 2 * FAMILY_MB)
    off = ys.astype(np.int64) * W + xs + ps * spp
    dec = Decisions(len(xs))
    tab_cam = type("T", (), {"cam4": cam4})()
    cx, cy, _ = camera_samples(tab_cam, alpha, W, H, spp, xs, ys, ps, dec)
    D = oracle_camera_rays(oracle, cam4, cx, cy)
    u2 = sampler(alpha, off, 2, dec)[0]
    sphs, tris, uvs = [], [], []
    big_tex = (1, 1001, 1001, (0.9, 0.8, 0.7), (0.2, 0.3, 0.4))
    textures = [(0, 1, 1, (0.7, 0.6, 0.5), (0, 0, 0)), big_tex, (0, 1, 1, (0.9, 0.85, 0.8), (0, 0, 0))]
    materials = [(MAT_LAMBERTIAN, 0, 0.0, (0, 0, 0)), (MAT_LAMBERTIAN, 1, 0.0, (0, 0, 0)), (MAT_DIELECTRIC, 0, 1.5, (0, 0, 0)),
                 (MAT_METAL, 2, 0.0, (0, 0, 0)), (MAT_LAMBERTIAN, 1, 0.0, (2.0, 1.5, 1.0)), (MAT_LAMBERTIAN, 0, 0.0, (0.0, 0.0, 0.0)),
                 (MAT_METAL, 2, 0.0, (1.0, 0.8, 0.6)), (MAT_METAL, 0, 0.0, (0, 0, 0))]
    bg = "sky"
    width_minus_1 = _MP.mpf(big_tex[1] - 1)
    for k in range(len(xs)):
        d = [_MP.mpf(float(x)) for x in D[k]]
        dn = _mnorm(d)
        t0 = _MP.mpf(rng.uniform(1.0, 2.5))
        P = [t0 * x for x in d]
        rho = t0 * _MP.mpf(0.3) / 64  # neighbouring sampled rays are >= 1 pixel = t0 / 64 apart at this depth
        rot = _MP.mpf(rng.uniform(0, 6.283))
        if name == "pole":
            s = 1 if k % 2 == 0 else -1  # facing the camera / facing away (then the shading normal is -g)
            zt = 1 - _MP.mpf(1e-9) + _offset(rng, 6e-14, 8e-13)
            ph = _MP.mpf(rng.uniform(0, 6.283))
            r = _MP.sqrt(1 - zt * zt)
            g = [r * _MP.cos(ph), r * _MP.sin(ph), zt * s]
            tris.append((*_tri_around(P, g, rho, rot), 0))
            uvs.append((0, 0, 1, 0, 0, 1))
        elif name in ("checker_tri", "emit_sky", "emit_black"):
            g = _mnorm([-dn[0] + _MP.mpf(rng.uniform(-0.3, 0.3)), -dn[1] + _MP.mpf(rng.uniform(-0.3, 0.3)), -dn[2]])
            a, b, c = _tri_around(P, g, rho, rot)
            ex = X.tri_exact(a, b, c, (0.0, 0.0, 0.0), D[k])
            ev = X.tri_prepass(np.array([a]), np.array([b]), np.array([c]), np.zeros((1, 3)), D[k:k + 1])
            on_u = k % 2 == 0
            q, e = (ex["u"], ev["u"].e[0]) if on_u else (ex["v"], ev["v"].e[0])
            qm = _MP.mpf(q.numerator) / q.denominator
            q2 = ex["v"] if on_u else ex["u"]
            qo = _MP.mpf(q2.numerator) / q2.denominator
            kk = int(rng.integers(10, 900))
            # a few half-widths of the parity quantity on either side of the integer kk
            hw = kk * (e / float(qm) + 2.0 ** -50)
            target = kk + _MP.mpf(rng.uniform(-40, 40)) * _MP.mpf(hw)
            scale = float(target / (width_minus_1 * qm))
            other = float((int(rng.integers(10, 900)) + _MP.mpf(0.5)) / (width_minus_1 * qo))
            uv = (0.0, 0.0, scale, 0.0, 0.0, other) if on_u else (0.0, 0.0, other, 0.0, 0.0, scale)
            m = 1 if name == "checker_tri" else 4
            tris.append((a, b, c, m))
            uvs.append(uv)
        elif name == "checker_sph":
            r = rho * _MP.mpf(0.5)
            n0 = [-x for x in dn]
            rr = _MP.sqrt(n0[0] ** 2 + n0[2] ** 2)
            b0 = _MP.atan2(-n0[2], n0[0])
            if k % 2 == 0:  # tu (w - 1) on an integer
                tu0 = (_MP.pi + b0) * _MP.mpf(1.0 / (2.0 * PI))
                kk = int(_MP.nint(tu0 * width_minus_1))
                phi = (kk + _offset(rng, 5e-10, 8e-9)) / (width_minus_1 * _MP.mpf(1.0 / (2.0 * PI)))
                beta = phi - _MP.mpf(PI)
                n = [rr * _MP.cos(beta), n0[1], -rr * _MP.sin(beta)]
            else:  # tv (h - 1) on an integer
                th0 = _MP.acos(-n0[1])
                kk = int(_MP.nint(th0 * _MP.mpf(1.0 / PI) * width_minus_1))
                th = (kk + _offset(rng, 5e-10, 8e-9)) / (width_minus_1 * _MP.mpf(1.0 / PI))
                ro = _MP.sin(th)
                n = [ro * n0[0] / rr, -_MP.cos(th), ro * n0[2] / rr]
            # hit point on the ray where the outward normal is n: the centre is P - r n
            cen = [P[i] - r * n[i] for i in range(3)]
            sphs.append((*[float(x) for x in cen], float(r), 1))
        elif name in ("tir", "schlick"):
            p = _basis(dn)[0]
            sgn = 1 if rng.random() < 0.5 else -1
            p = [x * sgn for x in p]
            if name == "tir":  # back-facing: ratio = index, index s = 1 at c = sqrt(1 - 1 / index^2)
                ix = _MP.mpf(1.5)
                c = _MP.sqrt(1 - 1 / (ix * ix)) + _offset(rng, 3e-14, 6e-13)
                g = [c * dn[i] + _MP.sqrt(1 - c * c) * p[i] for i in range(3)]
            else:  # front-facing: ratio = 1 / index, schlick(c, ratio) = u of this sample
                ratio = 1 / _MP.mpf(1.5)
                r0 = ((1 - ratio) / (1 + ratio)) ** 2
                uu = _MP.mpf(float(u2[k])) + _offset(rng, 3e-12, 6e-11)
                c = 1 - ((uu - r0) / (1 - r0)) ** (_MP.mpf(1) / 5) if uu > r0 + _MP.mpf(0.01) else _MP.mpf(0.5)
                g = [-c * dn[i] + _MP.sqrt(1 - c * c) * p[i] for i in range(3)]
            tris.append((*_tri_around(P, g, rho * 2, rot), 2))
            uvs.append((0, 0, 1, 0, 0, 1))
        elif name == "pole_bottom":
            # first hit: an emissive mirror at P sending the ray back towards +z, to Q = P + L (x - d), x a unit
            # vector across the image's columns (perpendicular to d), L half the spacing of the sampled columns;
            # second hit: a metal triangle at Q whose shading normal has z = -(1 - 1e-9) + a few half-widths.  The
            # radiance at max_bounces 2 is fma(k2, emit_mirror, 0) with k2 = a + (1 - a) pow5(1 - omega_i.z), and
            # omega_i.z = -(r . n) differs between the two branches by ~|r_xy| |n_xy| ~ 4e-5.
            xl = _mnorm(_mcross(dn, [_MP.mpf(0), _MP.mpf(1), _MP.mpf(0)]))
            L = t0 / 16
            r = _mnorm([xl[i] - dn[i] for i in range(3)])
            Q = [P[i] + L * (xl[i] - dn[i]) for i in range(3)]
            m = _mnorm([r[i] - dn[i] for i in range(3)])  # the mirror's normal: reflect(d) = r
            tris.append((*_tri_around(P, m, t0 / 200, rot), 6))
            uvs.append((0, 0, 1, 0, 0, 1))
            zt = -(1 - _MP.mpf(1e-9)) + _offset(rng, 6e-14, 8e-13)
            ph = _MP.mpf(rng.uniform(0, 6.283))
            rr = _MP.sqrt(1 - zt * zt)
            n = [rr * _MP.cos(ph), rr * _MP.sin(ph), zt]
            s = 1 if k % 2 == 0 else -1  # the triangle faces r (g = n) or away from it (g = -n, flipped back to n)
            tris.append((*_tri_around(Q, [s * x for x in n], t0 / 200, rot), 7))
            uvs.append((0, 0, 1, 0, 0, 1))
        elif name == "metal_grazing":
            r0 = rho * _MP.mpf(0.4)
            p = _basis(dn)[0]
            gam = _MP.mpf(10.0 ** rng.uniform(-5.6, -4.5))  # omega_i.z at the hit
            cen = [float(P[i] + r0 * p[i]) for i in range(3)]
            # exact impact parameter of the rounded centre: b^2 = |f|^2 - (f.d)^2 / |d|^2
            f = [_MP.mpf(cen[i]) for i in range(3)]
            dd = [_MP.mpf(float(x)) for x in D[k]]
            fd = sum(f[i] * dd[i] for i in range(3))
            b2 = sum(x * x for x in f) - fd * fd / sum(x * x for x in dd)
            rad = float(_MP.sqrt(b2 / (1 - gam * gam)))
            sphs.append((*cen, rad, 3))
    if name == "emit_black":
        bg = "black"
        # an enclosure around the camera (off-centre: b' = 0 would tie the sphere's roots): every second segment
        # ends on a grey, non-emissive wall
        sphs.append((1.3, -0.7, 2.1, 40.0, 5))
        materials[5] = (MAT_LAMBERTIAN, 2, 0.0, (0.0, 0.0, 0.0))
    uv = np.array(uvs, dtype=np.float64).reshape(-1) if uvs else None
    d, keep = make_scene_desc(abi, sphs, tris, uv, materials, textures, bg)
    return C.pointer(d), (d, keep), W, H, spp, xs, ys, ps
