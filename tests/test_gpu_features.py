"""ptx_render_features_device: the first-hit feature sums (albedo, normal, depth, hits).

Per sample -- one pass into a zeroed buffer is that pass's record: hits and depth equal the oracle's closest hit of the oracle's
camera ray bit for bit, normal and albedo lie inside the enclosures of tests/feature_reference.py (built from exact_shading's
primitives), and a Lambertian hit's albedo is ptx_debug_first_scatter's attenuation bit for bit.  Sums -- [0, N) is the sequential
binary64 sum of the single-pass buffers, any partition into slices at any passes_per_batch gives the same bits, and so does a second
run.  Scenes: Shirley (Simd_leaf and Array_leaf, tree in LDS), cornell (triangles, spheres, an emitter), a ganesha-like mesh of 3k
triangles on a floor, and one of 40k walked from HBM / L2."""
import ctypes as C
import types

import numpy as np
import pytest

import exact_shading as S
import feature_reference as FR

gpu = pytest.mark.gpu
N, DEPTH, NS = 4, 2, 1500
STOCK = ["shirley", "shirley_no_simd", "cornell", "ganesha_3k"]
MESH = "ganesha_40k"
_CACHE = {}


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


@pytest.fixture(scope="module")
def P():
    import path_tracer_ocaml_amd as P
    assert P.lib().ptx_device_count() >= 1, P.last_error()
    return P


@pytest.fixture(scope="module")
def torch():
    return pytest.importorskip("torch")


def desc_of(name, oracle):
    from path_tracer_ocaml_amd import abi
    if name == MESH:
        d = oracle.desc_ganesha_like(64, 36, n_target=40000)
        return d.ptr, d, 64, 36
    ptr, keep, W, H, _ = S.stock_desc(name, oracle, abi)
    return ptr, keep, W, H


def reference(name, oracle):
    """Built once per scene and left unchanged: the samples, the oracle's camera rays and closest hits, and (stock scenes) the
    enclosures of the feature record."""
    if name not in _CACHE:
        ptr, keep, W, H = desc_of(name, oracle)
        xs, ys, ps = S.random_samples(name, W, H, N, n=NS)
        enc = None
        if name == MESH:
            cam = ptr.contents.camera
            tab = types.SimpleNamespace(cam4=np.array([cam.lower_left_x, cam.lower_left_y, cam.view_x, cam.view_y]))
            cx, cy, _ = S.camera_samples(tab, S.lds_alpha(oracle, 2 + 2 * DEPTH), W, H, N, xs, ys, ps, S.Decisions(NS))
            D = S.oracle_camera_rays(oracle, tab.cam4, cx, cy)
        else:
            smp = S.Samples(oracle, S.Tables(ptr), W, H, N, DEPTH, xs, ys, ps)
            enc = FR.enclosures(smp)
            D = smp.D
        sc = oracle.Scene(ptr, keep)
        t, prim, _ = sc.intersect_rays(np.zeros_like(D), D)
        sc.close()
        _CACHE[name] = dict(ptr=ptr, keep=keep, W=W, H=H, xs=xs, ys=ys, ps=ps, D=D, t=t, prim=prim, enc=enc)
    return _CACHE[name]


@pytest.mark.parametrize("name", STOCK)
def test_the_restatement_is_robust_on_the_stock_scenes(oracle, name):
    """at most 1 % of the samples may be left out of the enclosure checks (here: none are)"""
    enc = reference(name, oracle)["enc"]
    skipped = int((~enc["robust"]).sum())
    print(f"\n{name}: {skipped} of {NS} samples not robust")
    assert skipped <= NS // 100


def _feat(torch, H, W):
    return torch.zeros((H, W, 8), dtype=torch.float64, device="cuda:0")


def _single_passes(P, torch, g, W, H, **kw):
    params = P.render_params(W, H, N, DEPTH, **kw)
    out = []
    for p in range(N):
        f = _feat(torch, H, W)
        st = g.render_features_device(params, p, 1, f.data_ptr())
        assert st["samples"] == W * H
        out.append(f.cpu().numpy())
    return np.stack(out)


def _first_scatter(P, g, W, H, xs, ys, ps):
    from path_tracer_ocaml_amd import abi
    n = len(xs)
    ip, dp = P.ip, P.dp
    G = P.lib()
    G.ptx_debug_first_scatter.argtypes = [C.c_void_p, C.POINTER(abi.RenderParams), C.c_int64, ip, ip, ip, dp, dp, ip]
    ray, att, alive = np.zeros((n, 6)), np.zeros((n, 3)), np.zeros(n, np.int32)
    xs, ys, ps = (np.ascontiguousarray(a, dtype=np.int32) for a in (xs, ys, ps))
    params = P.render_params(W, H, N, DEPTH)
    rc = G.ptx_debug_first_scatter(g._h, C.byref(params), n, xs.ctypes.data_as(ip), ys.ctypes.data_as(ip), ps.ctypes.data_as(ip),
                                   ray.ctypes.data_as(dp), att.ctypes.data_as(dp), alive.ctypes.data_as(ip))
    assert rc == 0, P.last_error()
    return att, alive


@gpu
@pytest.mark.parametrize("name", STOCK + [MESH])
def test_per_sample_records(P, torch, oracle, name):
    r = reference(name, oracle)
    W, H, xs, ys, ps = r["W"], r["H"], r["xs"], r["ys"], r["ps"]
    g = P.Scene(r["ptr"], 0, keepalive=r["keep"])
    try:
        in_lds = g.stats()["traversal_in_lds"]
        assert in_lds == {"shirley": 1, "shirley_no_simd": 1, "cornell": 1, MESH: 0}.get(name, in_lds)
        singles = _single_passes(P, torch, g, W, H)
        att, alive = _first_scatter(P, g, W, H, xs, ys, ps) if name != MESH else (None, None)
    finally:
        g.close()
    rec = singles[ps, ys, xs]
    hit = r["prim"] >= 0
    assert hit.any()
    # hits and depth: the oracle's closest hit of the oracle's camera ray, bit for bit
    assert np.array_equal(rec[:, 7], hit.astype(np.float64))
    assert np.array_equal(bits(rec[hit, 6]), bits(r["t"][hit])), f"{int((bits(rec[hit, 6]) != bits(r['t'][hit])).sum())} depths differ"
    assert (rec[~hit, 6] == 0.0).all() and (rec[~hit, 3:6] == 0.0).all()
    # a hit's normal is a unit vector (to rounding) on every scene
    assert np.abs(np.linalg.norm(rec[hit, 3:6], axis=1) - 1.0).max() < 1e-14
    if name == MESH:
        _check_mesh_against_the_description(r, rec, hit)
        return
    enc = r["enc"]
    rob = enc["robust"]
    assert np.array_equal(enc["hit"][rob], hit[rob])
    h, m = rob & hit, rob & ~hit
    bad_n = h & ~S.inside(enc["normal"], rec[:, 3:6])
    assert not bad_n.any(), f"{int(bad_n.sum())} normals outside their enclosure, first {np.nonzero(bad_n)[0][:5]}"
    assert np.array_equal(bits(rec[h, 0:3]), bits(enc["albedo"][h])), "albedo of a hit is not the texture colour"
    bad_b = m & ~S.inside(enc["bg"], rec[:, 0:3])
    assert not bad_b.any(), f"{int(bad_b.sum())} background colours outside their enclosure"
    # a Lambertian hit that scattered: the attenuation of the first scatter is the texture colour (pd / pd = 1)
    lam = hit & (alive == 1) & _lambertian(r, oracle)
    assert lam.sum() > 100 or name == "ganesha_3k"
    assert np.array_equal(bits(rec[lam, 0:3]), bits(att[lam]))


def _check_mesh_against_the_description(r, rec, hit):
    """The mesh walked from HBM / L2, without the exact restatement (40k triangles): a hit's normal is the geometric normal of the
    oracle's primitive turned against the ray -- a plain numpy cross product, so to 1e-12 and not to the bit -- and its albedo is,
    bit for bit, one of the two colours of that primitive's texture ((1, 1, 1) for a dielectric); a miss shows the background."""
    tab = S.Tables(r["ptr"])
    prim = np.where(hit, r["prim"], 0)
    A, B, Cc = S._prim_vertices(tab, prim)
    gn = np.cross(B - A, Cc - A)
    gn /= np.linalg.norm(gn, axis=1)[:, None]
    gn = np.where((np.einsum("ij,ij->i", r["D"], gn) < 0.0)[:, None], gn, -gn)
    tri = hit & ~tab.is_sphere(prim)
    assert tri.sum() > 100 and tri.sum() == hit.sum()  # a mesh on a floor: no spheres
    assert np.abs(rec[tri, 3:6] - gn[tri]).max() < 1e-12
    mat = tab.mat[prim]
    tex = np.clip(tab.m_tex[mat], 0, len(tab.t_kind) - 1)
    die = tab.m_kind[mat] == S.MAT_DIELECTRIC
    even = np.where(die[:, None], 1.0, tab.t_even[tex])
    odd = np.where(die[:, None] | (tab.t_kind[tex] == 0)[:, None], even, tab.t_odd[tex])
    is_even = (bits(rec[:, 0:3]) == bits(even)).all(axis=1)
    is_odd = (bits(rec[:, 0:3]) == bits(odd)).all(axis=1)
    assert (is_even | is_odd)[hit].all(), f"{int((~(is_even | is_odd))[hit].sum())} albedos are not a colour of the hit texture"
    if tab.bg_kind == 0:
        assert (rec[~hit, 0:3] == 0.0).all()
    else:
        d = r["D"][~hit]
        t = 0.5 * (d[:, 1] / np.linalg.norm(d, axis=1) + 1.0)
        sky = (1.0 - t)[:, None] * tab.horizon + t[:, None] * tab.zenith
        assert np.abs(rec[~hit, 0:3] - sky).max() < 1e-12


def _lambertian(r, oracle):
    """per sample: the oracle's closest hit is on a Lambertian material (from the description, not from the restatement)"""
    tab = S.Tables(r["ptr"])
    prim = np.where(r["prim"] >= 0, r["prim"], 0)
    return (r["prim"] >= 0) & (tab.m_kind[tab.mat[prim]] == S.MAT_LAMBERTIAN)


@gpu
@pytest.mark.parametrize("name", STOCK + [MESH])
def test_sums_in_pass_order_slices_batches_and_runs(P, torch, oracle, name):
    r = reference(name, oracle)
    W, H = r["W"], r["H"]
    g = P.Scene(r["ptr"], 0, keepalive=r["keep"])
    try:
        singles = _single_passes(P, torch, g, W, H)
        want = np.zeros((H, W, 8))
        for p in range(N):
            want = want + singles[p]
        rng = np.random.default_rng(5)
        parts = [[(0, N)], [(0, N)], [(k, k + 1) for k in range(N)]]
        for _ in range(3):
            cuts = sorted(rng.choice(np.arange(1, N), size=int(rng.integers(1, N)), replace=False).tolist())
            edges = [0] + cuts + [N]
            parts.append(list(zip(edges[:-1], edges[1:])))
        for ppb in (0, 1, 3):
            params = P.render_params(W, H, N, DEPTH, passes_per_batch=ppb)
            for part in parts:
                f = _feat(torch, H, W)
                for a, b in part:
                    st = g.render_features_device(params, a, b - a, f.data_ptr())
                    assert st["samples"] == W * H * (b - a)
                assert np.array_equal(bits(f.cpu().numpy()), bits(want)), (name, ppb, part)
        # the buffer is added to, never zeroed
        f = torch.full((H, W, 8), 2.0, dtype=torch.float64, device="cuda:0")
        g.render_features_device(P.render_params(W, H, N, DEPTH), 1, 1, f.data_ptr())
        assert np.array_equal(bits(f.cpu().numpy()), bits(2.0 + singles[1]))
        # one GPU, whole image: refused by the library itself
        from path_tracer_ocaml_amd import abi
        for kw in ({"band_step": 2, "band_rows": 8}, {"n_gpus": 2}):
            bad = P.render_params(W, H, N, DEPTH, **kw)
            f = _feat(torch, H, W)
            rc = P.lib().ptx_render_features_device(g._h, C.byref(bad), 0, 1, C.c_void_p(f.data_ptr()), None, C.byref(abi.Stats()))
            assert rc == -1 and "one GPU" in P.last_error()  # PTX_ERR_ARG
            assert float(f.abs().max()) == 0.0
    finally:
        g.close()


@gpu
def test_async_slices_on_a_stream(P, torch, oracle):
    r = reference("cornell", oracle)
    W, H = r["W"], r["H"]
    g = P.Scene(r["ptr"], 0, keepalive=r["keep"])
    try:
        whole = _feat(torch, H, W)
        g.render_features_device(P.render_params(W, H, N, DEPTH), 0, N, whole.data_ptr())
        s = torch.cuda.Stream()
        f = _feat(torch, H, W)
        torch.cuda.synchronize()
        params = P.render_params(W, H, N, DEPTH, asynchronous=True, passes_per_batch=1)
        for a, b in ((0, 1), (1, 3), (3, 4)):
            g.render_features_device(params, a, b - a, f.data_ptr(), stream=s.cuda_stream)
        s.synchronize()
        assert torch.equal(f.view(torch.int64), whole.view(torch.int64))
    finally:
        g.close()


@gpu
@pytest.mark.parametrize("W,H", [(1, 1), (1, 37), (37, 1)])
def test_edge_sizes_and_pass_ranges(P, torch, oracle, W, H):
    d = oracle.desc_shirley(W, H)
    g = P.Scene(d.ptr, 0, keepalive=d)
    try:
        params = P.render_params(W, H, N, DEPTH)
        whole = _feat(torch, H, W)
        g.render_features_device(params, 0, N, whole.data_ptr())
        acc = np.zeros((H, W, 8))
        for p in range(N):
            f = _feat(torch, H, W)
            g.render_features_device(params, p, 1, f.data_ptr())
            one = f.cpu().numpy()
            assert set(np.unique(one[..., 7])) <= {0.0, 1.0}
            acc = acc + one
        assert np.array_equal(bits(whole.cpu().numpy()), bits(acc))
        # against the oracle's closest hits of pass 0
        xs, ys = (a.ravel() for a in np.meshgrid(np.arange(W), np.arange(H)))
        cam = d.ptr.contents.camera
        tab = types.SimpleNamespace(cam4=np.array([cam.lower_left_x, cam.lower_left_y, cam.view_x, cam.view_y]))
        cx, cy, _ = S.camera_samples(tab, S.lds_alpha(oracle, 2 + 2 * DEPTH), W, H, N, xs, ys, np.zeros_like(xs), S.Decisions(len(xs)))
        D = S.oracle_camera_rays(oracle, tab.cam4, cx, cy)
        sc = oracle.Scene(d.ptr, d)
        t, prim, _ = sc.intersect_rays(np.zeros_like(D), D)
        sc.close()
        f = _feat(torch, H, W)
        g.render_features_device(params, 0, 1, f.data_ptr())
        one = f.cpu().numpy()[ys, xs]
        assert np.array_equal(one[:, 7], (prim >= 0).astype(np.float64))
        assert np.array_equal(bits(one[prim >= 0, 6]), bits(t[prim >= 0]))
        f = _feat(torch, H, W)
        for a, n in ((-1, 2), (0, 0), (N - 1, 2), (N, 1), (0, N + 1), (2, -1)):
            with pytest.raises(P.PtxError, match="pass"):
                g.render_features_device(params, a, n, f.data_ptr())
        assert float(f.abs().max()) == 0.0
    finally:
        g.close()
