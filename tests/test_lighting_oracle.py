"""The lighting rule as an estimator, on the CPU: the restatement tests/c/lighting_oracle.c and the light
table the library builds for host-only scenes.

  * ptx_scene_lighting's count and area are the restatement's;
  * the light half's pdf integrates to one over the sphere of directions;
  * mode 0 of the restatement is the oracle's orc_trace_samples bit for bit;
  * path-order accumulation makes cosine and mixture sampling estimate the same frame mean (|z| <= 4, the normal tail bound
    6e-5 -- the inputs are deterministic), and the reference's formula does not: that is why mode 1 exists;
  * the mixture samples the lamp: the median per-pixel variance drops by far more than a factor 20.
"""
import numpy as np
import pytest

import exact_geometry as X
import lighting_support as S

W = H = 48
DEPTH = 8
SPP = 256


@pytest.fixture(scope="module")
def P():
    import path_tracer_ocaml_amd as P
    return P


@pytest.fixture(scope="module")
def traced():
    """per scene and mode: (frame mean, standard error, per-pixel variance) of the 48 x 48 x 256 samples, traced once"""
    cache = {}

    def get(name, mode):
        if (name, mode) not in cache:
            hs = S.host_scene(name, W, H)
            r = S.Restatement(hs.ptr, hs)
            xs, ys, ps = S.all_samples(W, H, SPP)
            cache[(name, mode)] = S.frame_stats(r.trace_samples(mode, W, H, SPP, DEPTH, xs, ys, ps), W * H, SPP)
            r.close()
        return cache[(name, mode)]
    return get


@pytest.mark.parametrize("name", list(S.SCENES))
def test_light_table_matches_the_restatement(P, name):
    hs = S.host_scene(name, W, H)
    n, area, table = S.Restatement(hs.ptr, hs).lights()
    assert n == 2
    g = P.Scene(hs.ptr, -1, keepalive=hs)  # host-only: no GPU needed
    assert g.lighting() == (0, 0, 0.0)
    g.set_lighting("path-order")
    assert g.lighting() == (1, 0, 0.0)  # the list is built when mode 2 is first set
    g.set_lighting("sampled")
    mode, gn, garea = g.lighting()
    assert (mode, gn) == (2, 2)
    assert np.float64(garea).view(np.uint64) == np.float64(area).view(np.uint64)
    assert area == table[-1, 13] and np.isclose(area, {"ceiling12": 1.0}.get(name, area))
    g.set_lighting("reference")
    assert g.lighting() == (0, 2, garea)  # sticky mode, the list stays
    g.close()


def test_stock_cornell_from_the_oracle_desc(P, oracle):
    d = oracle.desc_cornell(W, H)
    n, area, _ = S.Restatement(d.ptr, d).lights()
    g = P.Scene(d.ptr, -1, keepalive=d)
    g.set_lighting(P.abi.PTX_LIGHTING_SAMPLED)
    assert g.lighting() == (2, 2, area) and n == 2


def test_scenes_without_an_emissive_tree_triangle(P, oracle):
    d = oracle.desc_shirley(96, 48)
    assert S.Restatement(d.ptr, d).lights()[0] == 0
    g = P.Scene(d.ptr, -1, keepalive=d)
    with pytest.raises(P.PtxError, match=r"\(-1\).*emissive triangle"):
        g.set_lighting("sampled")
    assert g.lighting() == (0, 0, 0.0)
    g.set_lighting("path-order")  # allowed: there is no emission to order, it renders as mode 0
    assert g.lighting()[0] == 1
    with pytest.raises(P.PtxError, match="unknown lighting mode"):
        P._check(P.lib().ptx_scene_set_lighting(g._h, 3))
    # an emissive SPHERE is not sampled either
    mats = [(0, 0, 0.0, (0, 0, 0)), (0, 0, 0.0, (5.0, 5.0, 5.0))]
    dd, keep = X.make_desc(P.abi, spheres=[(0, 0, -3, 1.0, 1)], tris=[((-1, -1, -2), (1, -1, -2), (0, 1, -2), 0)], materials=mats,
                           textures=[(0, 1, 1, (0.5, 0.5, 0.5), (0, 0, 0))])
    g2 = P.Scene(dd, -1, keepalive=keep)
    with pytest.raises(P.PtxError, match="emissive triangle"):
        g2.set_lighting("sampled")


@pytest.mark.parametrize("n_tri,ok", [(64, True), (65, False)])
def test_the_light_list_holds_at_most_64_triangles(P, n_tri, ok):
    mats = [(0, 0, 0.0, (0, 0, 0)), (0, 0, 0.0, (2.0, 2.0, 2.0))]
    tris = [((0.1 * k, 0.0, -2.0), (0.1 * k + 0.1, 0.0, -2.0), (0.1 * k, 0.1, -2.0), 1) for k in range(n_tri)]
    tris.append(((-5, -1, -9), (5, -1, -9), (0, 5, -9), 0))
    dd, keep = X.make_desc(P.abi, tris=tris, materials=mats, textures=[(0, 1, 1, (0.5, 0.5, 0.5), (0, 0, 0))])
    assert S.Restatement(C_ptr(P, dd), keep).lights()[0] == n_tri
    g = P.Scene(dd, -1, keepalive=keep)
    if ok:
        g.set_lighting("sampled")
        mode, n, area = g.lighting()
        assert (mode, n) == (2, 64) and np.isclose(area, 64 * 0.005)
    else:
        with pytest.raises(P.PtxError, match=r"\(-1\).*PTX_MAX_LIGHT_TRIANGLES"):
            g.set_lighting("sampled")
        assert g.lighting() == (0, 0, 0.0)


def C_ptr(P, desc):
    import ctypes
    return ctypes.pointer(desc)


@pytest.mark.parametrize("name", ["ceiling12", "lamp012"])
def test_the_light_pdf_is_a_density(name):
    """4 pi * mean(light_pd) over uniform directions = the integral of the density over the sphere = 1, from eight points at least
    0.2 away from the light's plane (closer, t^2 / |cos| is heavy-tailed and the standard error stops meaning much) and not
    coplanar with it."""
    hs = S.host_scene(name, W, H)
    r = S.Restatement(hs.ptr, hs)
    _, _, table = r.lights()
    # the scene lives in camera space: build the points from the light itself (a point of its plane, its normal, an edge)
    a, b, nrm = table[0, 0:3], table[0, 3:6], table[0, 9:12]
    centre = (table[0, 0:3] + table[0, 6:9]) / 2.0
    e1 = (b - a) / np.linalg.norm(b - a)
    e2 = np.cross(nrm, e1)
    rng = np.random.default_rng(20261016)
    n_dir = 1 << 20
    ws = rng.normal(size=(n_dir, 3))
    ws /= np.linalg.norm(ws, axis=1, keepdims=True)
    pts = [centre + d * nrm * s + ox * e1 + oy * e2
           for (d, ox, oy), s in zip([(0.2, 0.0, 0.0), (0.25, 0.1, -0.1), (0.3, -0.2, 0.15), (0.4, 0.3, 0.3), (0.5, 0.0, 0.2), (0.6, -0.3, -0.2),
                                      (0.75, 0.1, 0.1), (0.9, -0.1, 0.3)], [1, -1, 1, -1, 1, -1, 1, -1])]
    for p in pts:
        assert abs(np.dot(p - centre, nrm)) >= 0.2 - 1e-12
        pd = r.light_pd_many(p, ws)
        est = 4.0 * np.pi * pd.mean()
        se = 4.0 * np.pi * pd.std(ddof=1) / np.sqrt(n_dir)
        print(f"{name} p={np.round(p, 3)} integral={est:.5f} +- {se:.5f}  z={(est - 1.0) / se:+.2f}")
        assert abs(est - 1.0) <= 4.0 * se, (p, est, se)
    assert r.light_pd(pts[0], ws[0]) == r.light_pd_many(pts[0], ws[:1])[0]


@pytest.mark.parametrize("name", ["ceiling12", "lamp003"])
@pytest.mark.parametrize("depth", [1, 2, 8, 16])
def test_mode_0_is_the_oracle(name, depth):
    hs = S.host_scene(name, W, H)
    r = S.Restatement(hs.ptr, hs)
    xs, ys, ps = S.all_samples(W, H, 8)
    a = r.trace_samples(0, W, H, 8, depth, xs, ys, ps)
    b = r.trace_samples_oracle(W, H, 8, depth, xs, ys, ps)
    assert np.array_equal(a.view(np.uint64), b.view(np.uint64))
    assert a.max() > 0.0 or depth == 1


def test_mode_0_matches_the_shipped_oracle(oracle):
    """the included copy (math mode set to the shared functions) is the oracle the other tests use"""
    hs = S.host_scene("lamp012", W, H)
    xs, ys, ps = S.all_samples(W, H, 4)
    a = S.Restatement(hs.ptr, hs).trace_samples(0, W, H, 4, DEPTH, xs, ys, ps)
    b, _ = oracle.Scene(hs.ptr, hs).trace_samples(W, H, 4, DEPTH, xs, ys, ps)
    assert np.array_equal(a.view(np.uint64), b.view(np.uint64))


@pytest.mark.slow
@pytest.mark.parametrize("name", list(S.SCENES))
def test_cosine_and_mixture_sampling_agree_in_path_order(traced, name):
    m1, se1, _ = traced(name, 1)
    m2, se2, _ = traced(name, 2)
    z = (m1 - m2) / np.hypot(se1, se2)
    print(f"{name}: mode 1 {m1:.4f} +- {se1:.4f}, mode 2 {m2:.4f} +- {se2:.4f}, z = {z:+.2f}")
    assert abs(m1 - m2) <= 4.0 * np.hypot(se1, se2)
    assert m2 > 0.0


@pytest.mark.slow
def test_the_reference_formula_disagrees_with_the_mixture(traced):
    """Mode 0 against mode 2 on the ceiling scene FAILS the inequality the path-order modes pass: the reference's emission formula
    weights earlier hits by later attenuations, and an importance weight pd != 1 lands on the wrong terms."""
    m0, se0, _ = traced("ceiling12", 0)
    m2, se2, _ = traced("ceiling12", 2)
    print(f"mode 0 {m0:.4f} +- {se0:.4f}, mode 2 {m2:.4f} +- {se2:.4f}, z = {(m0 - m2) / np.hypot(se0, se2):+.1f}")
    assert not abs(m0 - m2) <= 4.0 * np.hypot(se0, se2)


@pytest.mark.slow
def test_the_mixture_samples_the_lamp(traced):
    _, _, v1 = traced("lamp003", 1)
    _, _, v2 = traced("lamp003", 2)
    both = (v1 > 0.0) & (v2 > 0.0)
    ratio = np.median(v1[both] / v2[both])
    print(f"pixels compared {int(both.sum())} of {v1.size}, median variance ratio {ratio:.1f}, p25 {np.percentile(v1[both] / v2[both], 25):.1f}")
    assert both.sum() >= 500
    assert ratio >= 20.0
