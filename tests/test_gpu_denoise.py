"""ptx_denoise_device against the numpy restatement of its rule (tests/denoise_reference.py) bit for bit, on seeded synthetic
images that reach every branch of the rule and on a real cornell frame; ptx_render_denoised against the chain of device calls it
is documented to be, update for update and bit for bit."""
import numpy as np
import pytest

import denoise_reference as R

pytestmark = pytest.mark.gpu


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


def _dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


def _zeros(torch, H, W, c=3):
    return torch.zeros((H, W, c), dtype=torch.float64, device="cuda:0")


def synthetic(W, H, kf, seed):
    """raw means, se and feature SUMS of kf passes: blocks of unit normals along the axes (orthogonal neighbours), random unit
    normals, part-hit pixels (shorter normals), all-miss pixels (normal 0, depth 0, hits 0), albedo channels on both sides of 2^-7,
    hit pixels at depth 0"""
    rng = np.random.default_rng(seed)
    mean = rng.uniform(0.01, 5.0, (H, W, 3)) * rng.choice([1.0, 1.0, 8.0], (H, W, 1))
    se = rng.uniform(1e-3, 1.5, (H, W, 3))
    se[rng.random((H, W)) < 0.1] *= 1e-3
    axes = np.eye(3)[rng.integers(0, 3, ((H + 5) // 6, (W + 5) // 6))]
    n = np.kron(axes, np.ones((6, 6, 1)))[:H, :W] * rng.choice([1.0, -1.0], (H, W, 1))
    free = rng.random((H, W)) < 0.3
    v = rng.normal(size=(H, W, 3))
    n[free] = (v / np.linalg.norm(v, axis=2, keepdims=True))[free]
    a = rng.uniform(0.1, 1.0, (H, W, 3))
    dark = rng.random((H, W, 3)) < 0.25
    a[dark] = rng.uniform(0.0, 2.0 ** -6, (H, W, 3))[dark]  # both sides of the demodulation threshold 2^-7
    a[rng.random((H, W)) < 0.02] = 2.0 ** -7                 # and the threshold itself
    z = rng.uniform(0.5, 20.0, (H, W))
    z[rng.random((H, W)) < 0.05] = 0.0
    hits = np.full((H, W), float(kf))
    part = rng.random((H, W)) < 0.15
    hits[part] = rng.integers(1, max(kf, 2), (H, W))[part]
    miss = rng.random((H, W)) < 0.2
    if H * W > 4:
        miss[: max(1, H // 5)] = True  # a band of sky
    hits[miss] = 0.0
    frac = hits / kf
    feat = np.zeros((H, W, 8))
    feat[..., 0:3] = a * kf
    feat[..., 3:6] = n * frac[..., None] * kf
    feat[..., 6] = z * frac * kf
    feat[..., 7] = hits
    return mean, se, feat


SIZES = [(1, 1), (1, 40), (40, 1), (33, 31), (70, 45)]


@pytest.mark.parametrize("levels", [0, 1, 2, 5])
@pytest.mark.parametrize("W,H", SIZES)
def test_denoise_device_equals_the_restatement(P, torch, W, H, levels):
    kf = 3
    mean, se, feat = synthetic(W, H, kf, seed=W * 100 + H)
    rng = np.random.default_rng(7)
    counts = rng.integers(2, 10, (H, W)).astype(np.int32)
    d_err, d_feat, d_counts = _dev(torch, se), _dev(torch, feat), _dev(torch, counts)
    for m in (0, 5):
        for demod in (True, False):
            for k in (6, counts):
                uniform = np.isscalar(k)
                raw = mean * (k if uniform else k[..., None])
                d_raw, d_out = _dev(torch, raw), _zeros(torch, H, W)
                settings = dict(levels=levels, normal_power_log2=m, demodulate=demod)
                P.denoise_device(0, W, H, settings, k if uniform else 0, kf, d_raw.data_ptr(), d_err.data_ptr(), d_feat.data_ptr(),
                                 d_out.data_ptr(), d_passes_ptr=None if uniform else d_counts.data_ptr())
                want = R.denoise(raw, se, feat, k, kf, levels=levels, normal_power_log2=m, flags=R.DEMODULATE if demod else 0)
                got = d_out.cpu().numpy()
                assert np.isfinite(got).all()
                diff = bits(got) != bits(want)
                assert not diff.any(), (W, H, levels, m, demod, uniform, int(diff.sum()), np.argwhere(diff)[:3])
                if levels == 0:
                    assert np.array_equal(bits(got), bits(raw))


@pytest.mark.parametrize("lds_steps", ["0", "2"])
@pytest.mark.parametrize("W,H", [(33, 31), (70, 45), (1, 40)])
def test_either_tap_fetch_gives_the_same_bits(P, torch, W, H, lds_steps, monkeypatch):
    """PTX_ATROUS_LDS = the largest step whose taps are read from an LDS copy of the tile and its halo (default 1; DESIGN.md
    section 8): 0 gathers at every step, 2 uses LDS at steps 1 and 2"""
    kf, k = 3, 6
    mean, se, feat = synthetic(W, H, kf, seed=W * 100 + H)
    raw = mean * k
    d_raw, d_err, d_feat, d_out = _dev(torch, raw), _dev(torch, se), _dev(torch, feat), _zeros(torch, H, W)
    monkeypatch.setenv("PTX_ATROUS_LDS", lds_steps)
    for levels in (1, 2, 5):
        P.denoise_device(0, W, H, dict(levels=levels), k, kf, d_raw.data_ptr(), d_err.data_ptr(), d_feat.data_ptr(), d_out.data_ptr())
        want = R.denoise(raw, se, feat, k, kf, levels=levels)
        assert np.array_equal(bits(d_out.cpu().numpy()), bits(want)), (W, H, levels)


def test_denoise_device_checks_its_arguments(P, torch):
    W, H = 8, 8
    z3, z8 = _zeros(torch, H, W), _zeros(torch, H, W, 8)
    out = _zeros(torch, H, W)
    from path_tracer_ocaml_amd import abi
    import ctypes as C
    L = P.lib()

    def call(dn, k=4, kf=2, raw=z3, dst=out, w=W):
        return L.ptx_denoise_device(0, w, H, C.byref(dn), k, None, kf, C.c_void_p(raw.data_ptr()), C.c_void_p(z3.data_ptr()),
                                    C.c_void_p(z8.data_ptr()), C.c_void_p(dst.data_ptr()), None)

    assert call(P.denoise_defaults()) == 0
    for field, value in (("levels", 9), ("levels", -1), ("normal_power_log2", -1), ("normal_power_log2", 9), ("flags", 2),
                         ("sigma_luminance", 0.0), ("sigma_depth", float("nan")), ("sigma_albedo", float("inf")),
                         ("sigma_albedo", -1.0)):
        dn = P.denoise_defaults()
        setattr(dn, field, value)
        assert call(dn) == -1, (field, value)
    assert call(P.denoise_defaults(), k=1) == -1 and "passes_done" in P.last_error()
    assert call(P.denoise_defaults(), kf=0) == -1
    assert call(P.denoise_defaults(), dst=z3) == -1
    assert call(P.denoise_defaults(), w=0) == -1


# ---------------------------------------------------------------- real frames
W, H, N = 64, 48, 16
DEPTH = 8


@pytest.fixture(scope="module")
def scenes(P, oracle):
    made = {"shirley": oracle.desc_shirley(W, H), "cornell": oracle.desc_cornell(W, H)}
    out = {k: (d, P.Scene(d.ptr, 0, keepalive=d)) for k, d in made.items()}
    yield out
    for _, g in out.values():
        g.close()


def by_hand(P, torch, g, K, F, settings, w=W, h=H, n=N, depth=DEPTH):
    """The chain ptx_render_denoised is documented to be: per update (k, rgb, err, feature sums, kf), all host copies"""
    params = P.render_params(w, h, n, depth)
    raw, sq, feat = _zeros(torch, h, w), _zeros(torch, h, w), _zeros(torch, h, w, 8)
    err, den, rgb = _zeros(torch, h, w), _zeros(torch, h, w), _zeros(torch, h, w)
    Fe = min(F, n) if F > 0 else n
    updates = []
    first = 0
    while first < n:
        count = min(K, n - first)
        g.render_passes_device(params, first, count, raw.data_ptr(), sq.data_ptr())
        k = first + count
        kf = min(Fe, k)
        if first < Fe:
            g.render_features_device(params, first, kf - first, feat.data_ptr())
        rel = P.pixel_error_device(0, w, h, k, raw.data_ptr(), sq.data_ptr(), err.data_ptr())
        P.denoise_device(0, w, h, settings, k, kf, raw.data_ptr(), err.data_ptr(), feat.data_ptr(), den.data_ptr())
        P.film_resolve_device(0, w, h, k, den.data_ptr(), rgb.data_ptr())
        updates.append(dict(k=k, rel=rel, rgb=rgb.cpu().numpy(), err=err.cpu().numpy(), feat=feat.cpu().numpy(), kf=kf,
                            raw=raw.cpu().numpy(), den=den.cpu().numpy()))
        first = k
    return updates


@pytest.mark.parametrize("F", [0, 8])
@pytest.mark.parametrize("K", [4, 16])
@pytest.mark.parametrize("kind", ["cornell", "shirley"])
def test_every_update_is_the_chain_made_by_hand(P, torch, scenes, kind, K, F):
    _, g = scenes[kind]
    settings = dict(feature_passes=F)
    want = by_hand(P, torch, g, K, F, settings)
    for count_work in (False, True):  # count_work: the loop queues the next slice only after the callback
        seen = []

        def on_update(k, rel, rgb, err):
            seen.append((k, rel, rgb.copy(), err.copy()))

        rgb, err, feat, done, st = g.render_denoised(W, H, N, DEPTH, K, denoise=settings, on_update=on_update, feat_out=True,
                                                     count_work=count_work)
        assert [s[0] for s in seen] == [u["k"] for u in want] and done == N
        assert st["samples"] == W * H * N
        for (k, rel, rgb_k, err_k), u in zip(seen, want):
            assert rel == u["rel"], (k, rel, u["rel"])
            assert np.array_equal(bits(rgb_k), bits(u["rgb"])), (kind, K, F, k, count_work)
            assert np.array_equal(bits(err_k), bits(u["err"])), (kind, K, F, k)
        assert np.array_equal(bits(rgb), bits(want[-1]["rgb"]))
        assert np.array_equal(bits(feat), bits(want[-1]["feat"] / float(want[-1]["kf"])))
        assert feat[..., 7].max() == 1.0
    # the filter did something: the denoised sums differ from the raw ones
    assert not np.array_equal(want[-1]["den"], want[-1]["raw"])


@pytest.mark.parametrize("kind", ["cornell", "shirley"])
def test_levels_zero_run_to_the_end_is_ptx_render(P, scenes, kind):
    _, g = scenes[kind]
    ref, _ = g.render(W, H, N, DEPTH)
    rgb, err, feat, done, _ = g.render_denoised(W, H, N, DEPTH, 4, denoise=dict(levels=0))
    assert done == N and feat is None
    assert np.array_equal(bits(rgb), bits(ref))


def test_a_callback_that_stops_leaves_its_update(P, torch, scenes):
    _, g = scenes["cornell"]
    want = by_hand(P, torch, g, 4, 8, dict(feature_passes=8))
    calls = []

    def on_update(k, rel, rgb, err):
        calls.append(k)
        return len(calls) == 2

    rgb, err, feat, done, st = g.render_denoised(W, H, N, DEPTH, 4, denoise=dict(feature_passes=8), on_update=on_update, feat_out=True)
    assert calls == [4, 8] and done == 8 and st["samples"] == W * H * 8
    assert np.array_equal(bits(rgb), bits(want[1]["rgb"]))
    assert np.array_equal(bits(err), bits(want[1]["err"]))
    assert np.array_equal(bits(feat), bits(want[1]["feat"] / 8.0))


def test_the_target_error_stops_the_render_on_the_undenoised_sums(P, torch, scenes):
    _, g = scenes["shirley"]
    want = by_hand(P, torch, g, 4, 0, {})
    target = 0.5 * (want[0]["rel"] + want[1]["rel"])
    assert want[0]["rel"] > target > want[1]["rel"]
    rgb, _, _, done, _ = g.render_denoised(W, H, N, DEPTH, 4, target_rel_err=target)
    assert done == 8
    assert np.array_equal(bits(rgb), bits(want[1]["rgb"]))


def test_set_lighting_is_refused_while_a_denoised_render_runs(P, scenes):
    _, g = scenes["cornell"]
    got = []

    def on_update(k, rel, rgb, err):
        try:
            g.set_lighting("path-order")
        except P.PtxError as e:
            got.append(str(e))
        return True

    g.render_denoised(W, H, N, DEPTH, 4, on_update=on_update)
    assert got and "-3" in got[0]  # PTX_ERR_STATE
    assert g.lighting()[0] == 0


def test_cornell_frame_equals_the_restatement_and_its_quality(P, torch, oracle):
    """cornell 64x64, N = 8, depth 8 (the CPU quality test's frame): the device's output is the restatement's on the device's own
    inputs bit for bit, so its linear RMSE ratio against the oracle's 512-spp mean is the restatement's number: < 0.5, and the
    CPU test's ratio (whose features come from a plain numpy restatement of the first hit, equal to rounding rather than bit for
    bit) to 1e-6."""
    import test_denoise_reference as T
    w = h = 64
    n, depth = 8, 8
    d = oracle.desc_cornell(w, h)
    g = P.Scene(d.ptr, 0, keepalive=d)
    try:
        u = by_hand(P, torch, g, n, 8, {}, w=w, h=h, n=n, depth=depth)[-1]
    finally:
        g.close()
    want = R.denoise(u["raw"], u["err"], u["feat"], n, 8)
    assert np.array_equal(bits(u["den"]), bits(want))
    sc = oracle.Scene(d.ptr, d)
    ref = sc.render(w, h, 512, depth, threads=4, want_raw=True)["raw"] / 512
    sc.close()
    noisy, den = T.rmse(u["raw"] / n, ref), T.rmse(u["den"] / n, ref)
    cpu_noisy, cpu_den = T.quality_ratio(oracle, d, w, h, n, depth)
    print(f"\ncornell 64x64 spp 8 on the GPU: noisy {noisy:.4f} denoised {den:.4f} ratio {den / noisy:.4f} (CPU {cpu_den / cpu_noisy:.4f})")
    assert den < 0.5 * noisy
    assert noisy == cpu_noisy
    assert abs(den / noisy - cpu_den / cpu_noisy) <= 1e-6 * (cpu_den / cpu_noisy)
