"""Enclosures of the first-hit feature record (ptx_render_features_device) of a sample set, assembled from the primitives of
tests/exact_shading.py: the exact closest hit of every camera ray, the hit parameters as intervals, the facing shading normal
(Sphere.hit / Triangle.Hit.to_hit, negated when hit_front is false) as an interval vector, the texture colour (Texture.eval, whose
checker parity is a decision) and the background of a miss as an interval vector.  Only samples whose every decision is robust are
to be compared: `robust` says which."""
import numpy as np

import exact_shading as S
from exact_shading import Decisions, Samples, background, hit_params, texture, vnormalize  # noqa: F401 (the named primitives)


def enclosures(smp):
    """smp: an exact_shading.Samples.  Returns a dict: robust (n,), hit (n,), prim (n,), normal (3 intervals; hits),
    albedo (n, 3) exact colours of the hits, bg (3 intervals; misses), dielectric (n,)."""
    tab, O, D, res = smp.tab, smp.O, smp.D, smp.res
    n = len(O)
    dec = Decisions(n)
    dec.robust &= smp.dec0.robust & res.robust & smp.camera_ok
    hit, sph, tri, t_iv, u_iv, v_iv = hit_params(tab, res, O, D)
    prim = np.where(hit, res.prim, 0)
    o3, d3 = S.V(*[S._pt(O[:, k]) for k in range(3)]), S.V(*[S._pt(D[:, k]) for k in range(3)])
    g = tab.geo
    cen = np.concatenate([np.zeros((g.n_tri, 3)), g.sph_c, np.zeros((g.n_floor, 3))])[np.clip(prim, 0, g.n_prims + g.n_floor - 1)] \
        if g.n_prims + g.n_floor else np.zeros((n, 3))
    ps = S.vadd(o3, S.vscale(d3, t_iv))  # Ray.point_at
    ns = vnormalize(S.vsub(ps, S.V(*[S._pt(cen[:, k]) for k in range(3)])))
    A, B, Cc = S._prim_vertices(tab, prim)
    a3, b3, c3 = (S.V(*[S._pt(P[:, k]) for k in range(3)]) for P in (A, B, Cc))
    gn = vnormalize(S.vcross(S.vsub(b3, a3), S.vsub(c3, a3)))
    w = (1.0 - u_iv) - v_iv
    uv = tab.uv[prim]
    tu_t = (S._pt(uv[:, 0]) * w + S._pt(uv[:, 2]) * u_iv) + S._pt(uv[:, 4]) * v_iv
    tv_t = (S._pt(uv[:, 1]) * w + S._pt(uv[:, 3]) * u_iv) + S._pt(uv[:, 5]) * v_iv
    n0 = S.vwhere(sph, ns, gn)
    front = ~dec.decide("hit_front", S.vdot(d3, n0), 0.0, hit)
    normal = S.vwhere(front, n0, S.vneg(n0))
    theta = S.iacos(-normal[1])
    phi = S.PI + S.iatan2(-normal[2], normal[0])
    tu = S.where(sph, phi * (1.0 / (2.0 * S.PI)), tu_t)
    tv = S.where(sph, theta * (1.0 / S.PI), tv_t)
    mat = tab.mat[prim]
    kind_m = np.where(hit, tab.m_kind[mat], -1)
    textured = hit & ((kind_m == S.MAT_LAMBERTIAN) | (kind_m == S.MAT_METAL))
    die = hit & (kind_m == S.MAT_DIELECTRIC)
    col = texture(tab, tab.m_tex[mat], tu, tv, dec, (), textured)
    dec.require_finite(tu, tv, active=textured & (tab.t_kind[np.clip(tab.m_tex[mat], 0, len(tab.t_kind) - 1)] == 1))
    dec.require_finite(*normal, active=hit)
    albedo = np.where(die[:, None], 1.0, col)
    return {"robust": dec.robust, "hit": hit, "prim": np.where(hit, res.prim, -1), "normal": normal, "albedo": albedo,
            "bg": background(tab, d3), "dielectric": die, "lambertian": hit & (kind_m == S.MAT_LAMBERTIAN)}
