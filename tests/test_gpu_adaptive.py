"""Adaptive sampling on the GPU, bit for bit where the data allows it.

A pixel that stops after n passes holds the pass-order prefix of its own N-pass sums (the sampler offset depends only on
(x, y, pass, N), integrator.ml:98), so
* the sums a pixel list receives (ptx_render_pixels_device) are ptx_render_passes_device's at those pixels, bit for bit;
* the film and the error with a count map are ptx_film_resolve_device / ptx_pixel_error_device where the map is uniform;
* ptx_render_adaptive's pass map is a numpy restatement of the rounds, computed from prefix sums, and its image is the film of
  the prefixes that map names.
Scenes: Shirley (Simd_leaf, tree in LDS), cornell with its emitter, a ganesha-like mesh walked from HBM.
"""
import os
import re
import subprocess

import numpy as np
import pytest

import update_reference as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H, N = 64, 48, 16
DEPTH = {"shirley": 8, "cornell": 16, "ganesha": 8}
KINDS = ["shirley", "cornell", "ganesha"]


def bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


@pytest.fixture(scope="module")
def P():
    import path_tracer_ocaml_amd as P
    assert P.lib().ptx_device_count() >= 1, P.last_error()
    return P


@pytest.fixture(scope="module")
def torch():
    return pytest.importorskip("torch")


@pytest.fixture(scope="module")
def scenes(P, oracle):
    made = {"shirley": oracle.desc_shirley(W, H), "cornell": oracle.desc_cornell(W, H),
            "ganesha": oracle.desc_ganesha_like(W, H, n_target=40000)}
    out = {k: (d, P.Scene(d.ptr, 0, keepalive=d)) for k, d in made.items()}
    assert out["shirley"][1].stats()["traversal_in_lds"]
    assert not out["ganesha"][1].stats()["traversal_in_lds"]
    yield out
    for _, g in out.values():
        g.close()


def _zeros(torch, rows=H, w=W):
    return torch.zeros((rows, w, 3), dtype=torch.float64, device="cuda:0")


def _dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


@pytest.fixture(scope="module")
def prefixes(P, torch, scenes):
    """{kind: {k: (S1, S2)}} -- ptx_render_passes_device's prefix sums after k passes, k = 1..N"""
    out = {}
    for kind, (_, g) in scenes.items():
        params = P.render_params(W, H, N, DEPTH[kind], passes_per_batch=3)
        raw, sq = _zeros(torch), _zeros(torch)
        out[kind] = {}
        for k in range(1, N + 1):
            g.render_passes_device(params, k - 1, 1, raw.data_ptr(), sq.data_ptr())
            out[kind][k] = (raw.cpu().numpy(), sq.cpu().numpy())
    return out


def _lists(rng):
    npix = W * H
    tile = [(ty * W + tx) for ty in range(8, 16) for tx in range(16, 24)]
    return {
        "all": np.arange(npix), "empty": np.zeros(0, dtype=np.int64), "one": np.array([W * 17 + 5]),
        "r63": rng.choice(npix, 63, replace=False), "r64": rng.choice(npix, 64, replace=False),
        "r65": rng.choice(npix, 65, replace=False), "half": rng.choice(npix, npix // 2, replace=False),
        "tile": np.array(tile), "reversed": np.arange(npix)[::-1].copy(),
    }


# ---------------------------------------------------------------- 1. pixel lists
@pytest.mark.parametrize("kind", KINDS)
def test_pixel_lists_equal_the_slices(P, torch, scenes, kind):
    _, g = scenes[kind]
    rng = np.random.default_rng(5)
    a, c = 3, 9  # passes [3, 12) of the 16-pass frame
    sentinel = -1.25
    for ppb in (0, 2, 5):
        params = P.render_params(W, H, N, DEPTH[kind], passes_per_batch=ppb)
        ref_raw, ref_sq = _zeros(torch), _zeros(torch)
        g.render_passes_device(params, a, c, ref_raw.data_ptr(), ref_sq.data_ptr())
        ref_raw, ref_sq = ref_raw.cpu().numpy().reshape(-1, 3), ref_sq.cpu().numpy().reshape(-1, 3)
        for i, (name, lst) in enumerate(_lists(rng).items()):
            with_sq = (i + ppb) % 2 == 0
            init = np.full((W * H, 3), sentinel)
            init[lst] = 0.0
            raw, sq = _dev(torch, init), _dev(torch, init)
            d_list = _dev(torch, lst.astype(np.int32))
            st = g.render_pixels_device(params, a, c, d_list.data_ptr() if len(lst) else 0, len(lst), raw.data_ptr(),
                                        sq.data_ptr() if with_sq else None)
            assert st["samples"] == len(lst) * c, (kind, ppb, name)
            got, got_sq = raw.cpu().numpy(), sq.cpu().numpy()
            assert np.array_equal(bits(got[lst]), bits(ref_raw[lst])), (kind, ppb, name)
            if with_sq:
                assert np.array_equal(bits(got_sq[lst]), bits(ref_sq[lst])), (kind, ppb, name)
            off = np.ones(W * H, dtype=bool)
            off[lst] = False
            assert (got[off] == sentinel).all() and (got_sq[off] == sentinel).all(), (kind, ppb, name)
            if not with_sq:
                assert (got_sq[lst] == 0.0).all()
    assert float(np.abs(ref_raw).max()) > 0.0


# ---------------------------------------------------------------- 2. a bad list
def test_a_bad_list_is_refused_and_leaves_the_sums_alone(P, torch, scenes):
    _, g = scenes["shirley"]
    params = P.render_params(W, H, N, 8)
    # one slack pixel on each side: an unguarded write to index -1 or W*H would land in the slack and be seen
    buf = torch.zeros(((W * H + 2) * 3,), dtype=torch.float64, device="cuda:0")
    sq = torch.zeros(((W * H + 2) * 3,), dtype=torch.float64, device="cuda:0")
    inner, inner_sq = buf.data_ptr() + 24, sq.data_ptr() + 24
    for bad in (-1, W * H):
        lst = _dev(torch, np.array([0, 5, bad, 7], dtype=np.int32))
        with pytest.raises(P.PtxError, match="outside"):
            g.render_pixels_device(params, 0, 4, lst.data_ptr(), 4, inner, inner_sq)
        torch.cuda.synchronize()
        assert float(buf.abs().max()) == 0.0 and float(sq.abs().max()) == 0.0, bad
    lst = _dev(torch, np.array([0, 5], dtype=np.int32))
    for a, n in ((-1, 2), (0, 0), (15, 2)):
        with pytest.raises(P.PtxError, match="pass"):
            g.render_pixels_device(params, a, n, lst.data_ptr(), 2, inner)
    with pytest.raises(P.PtxError, match="n_pixels"):
        g.render_pixels_device(params, 0, 2, lst.data_ptr(), W * H + 1, inner)
    with pytest.raises(P.PtxError, match="one GPU"):
        g.render_pixels_device(P.render_params(W, H, N, 8, band_step=2), 0, 2, lst.data_ptr(), 2, inner)
    assert float(buf.abs().max()) == 0.0
    # the handle renders after the refusals
    g.render_pixels_device(params, 0, 2, lst.data_ptr(), 2, inner)
    assert float(buf[:3].abs().max()) == 0.0 and float(buf[3:6].abs().max()) > 0.0


# ---------------------------------------------------------------- 3. film with counts
def _film_weights():
    coeff = [1, 4, 6, 4, 1]
    num = []
    for i in range(3):
        acc = 0
        for k in range(5):
            lo, hi = max(3 * k, 5 * i), min(3 * k + 3, 5 * i + 5)
            if hi > lo:
                acc += (hi - lo) * coeff[k]
        num.append(acc)
    w = [n / 3.0 for n in num]
    total = 0.0
    for v in w:
        total = total + v
    w = [v / total for v in w]
    return [w[j // 3] * w[j % 3] for j in range(9)]


def _np_film_counts(raw, passes):
    kw = _film_weights()
    out = np.zeros_like(raw)
    for y in range(H):
        for x in range(W):
            acc = np.zeros(3)
            k = 0
            for dy in (-1, 0, 1):
                for dx in (-1, 0, 1):
                    sy, sx = y - dy, x - dx
                    if 0 <= sy < H and 0 <= sx < W:
                        acc = acc + kw[k] * (raw[sy, sx] * (1.0 / passes[sy, sx]))
                    k += 1
            out[y, x] = np.sqrt(acc)
    return out


def _uniform_taps(passes):
    same = np.ones((H, W), dtype=bool)
    pad = np.pad(passes, 1, constant_values=-1)
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            nb = pad[1 + dy:1 + dy + H, 1 + dx:1 + dx + W]
            same &= (nb == -1) | (nb == passes)
    return same


def _count_maps(rng):
    blocks = np.repeat(np.repeat(rng.integers(1, N + 1, (H // 8, W // 8)), 8, axis=0), 8, axis=1)
    return [rng.integers(1, N + 1, (H, W)), blocks, np.where(rng.random((H, W)) < 0.9, 16, 4)]


def test_film_with_counts(P, torch, prefixes):
    rng = np.random.default_rng(7)
    raw_np = prefixes["cornell"][N][0]
    raw, rgb, want = _dev(torch, raw_np), _zeros(torch), _zeros(torch)
    for n in (1, 5, N):
        passes = _dev(torch, np.full((H, W), n, dtype=np.int32))
        P.film_resolve_counts_device(0, W, H, raw.data_ptr(), passes.data_ptr(), rgb.data_ptr())
        P.film_resolve_device(0, W, H, n, raw.data_ptr(), want.data_ptr())
        assert torch.equal(rgb.view(torch.int64), want.view(torch.int64)), n
    any_same = False
    for m in _count_maps(rng):
        passes = _dev(torch, m.astype(np.int32))
        P.film_resolve_counts_device(0, W, H, raw.data_ptr(), passes.data_ptr(), rgb.data_ptr())
        got = rgb.cpu().numpy()
        same = _uniform_taps(m)
        any_same = any_same or bool(same.any())
        assert (~same).any()
        for n in np.unique(m[same]):
            P.film_resolve_device(0, W, H, int(n), raw.data_ptr(), want.data_ptr())
            at = same & (m == n)
            assert np.array_equal(bits(got[at]), bits(want.cpu().numpy()[at])), n
        ref = _np_film_counts(raw_np, m)
        np.testing.assert_allclose(got[~same], ref[~same], rtol=1e-13, atol=0)
    assert any_same


# ---------------------------------------------------------------- 4. error with counts
def _np_error(s1, s2, k):
    k = k[..., None].astype(np.float64)
    se = np.where(k >= 2, np.sqrt(np.maximum(0.0, s2 - s1 * s1 / k) / (k * (k - 1))), np.inf)
    m = s1 / k
    return se, np.sqrt((se * se).sum()) / np.sqrt((m * m).sum())


def test_error_with_counts(P, torch, prefixes):
    rng = np.random.default_rng(9)
    s1, s2 = prefixes["shirley"][N]
    raw, sq, err, want = _dev(torch, s1), _dev(torch, s2), _zeros(torch), _zeros(torch)
    for n in (2, 7, N):
        passes = _dev(torch, np.full((H, W), n, dtype=np.int32))
        rel = P.pixel_error_counts_device(0, W, H, passes.data_ptr(), raw.data_ptr(), sq.data_ptr(), err.data_ptr())
        want_rel = P.pixel_error_device(0, W, H, n, raw.data_ptr(), sq.data_ptr(), want.data_ptr())
        assert torch.equal(err.view(torch.int64), want.view(torch.int64)), n
        assert np.float64(rel).view(np.uint64) == np.float64(want_rel).view(np.uint64), n
    for m in _count_maps(rng)[1:]:
        m = np.maximum(m, 2)
        passes = _dev(torch, m.astype(np.int32))
        rel = P.pixel_error_counts_device(0, W, H, passes.data_ptr(), raw.data_ptr(), sq.data_ptr(), err.data_ptr())
        se, want_rel = _np_error(s1, s2, m)
        np.testing.assert_allclose(err.cpu().numpy(), se, rtol=1e-12, atol=0)
        assert abs(rel - want_rel) <= 1e-12 * want_rel
    one = _dev(torch, np.where(np.arange(W * H).reshape(H, W) == 7, 1, 4).astype(np.int32))
    assert P.pixel_error_counts_device(0, W, H, one.data_ptr(), raw.data_ptr(), sq.data_ptr()) == float("inf")
    z = _zeros(torch)
    assert P.pixel_error_counts_device(0, W, H, passes.data_ptr(), z.data_ptr(), z.data_ptr()) == 0.0


# ---------------------------------------------------------------- 5. the rule, restated
def _restate(pref, M, K, T, F):
    """the pass map the rounds give, and each round's count of pixels for the next round (tests/update_reference.py)"""
    return R.restate_rounds(pref, W, H, N, M, K, T, F)


def _targets(pref, M, K, F):
    """two targets at least 1e-6 relative from every pixel's e / d at every round boundary"""
    return R.targets(pref, N, M, K, F)


_assembled = R.assembled


@pytest.mark.parametrize("kind", KINDS)
def test_rounds_follow_the_rule(P, torch, oracle, scenes, prefixes, kind):
    d, g = scenes[kind]
    pref = prefixes[kind]
    M = K = 4
    F = 1e-3
    if kind == "cornell":  # the prefixes are the oracle's per-sample radiance summed in pass order
        ys, xs, ps = np.meshgrid(np.arange(H), np.arange(W), np.arange(N), indexing="ij")
        rgb, _ = oracle.Scene(d.ptr, d).trace_samples(W, H, N, DEPTH[kind], xs.ravel(), ys.ravel(), ps.ravel())
        per = rgb.reshape(H, W, N, 3)
        s1, s2 = np.zeros((H, W, 3)), np.zeros((H, W, 3))
        for k in range(N):
            s1, s2 = s1 + per[:, :, k], s2 + per[:, :, k] * per[:, :, k]
            assert np.array_equal(bits(s1), bits(pref[k + 1][0])) and np.array_equal(bits(s2), bits(pref[k + 1][1])), k
    for T in _targets(pref, M, K, F):
        want, actives = _restate(pref, M, K, T, F)
        rounds = []
        rgb, err, passes, st = g.render_adaptive(W, H, N, DEPTH[kind], T, min_passes=M, passes_per_round=K, radiance_floor=F,
                                                 on_round=lambda *a: rounds.append(a[:5]))
        assert np.array_equal(passes, want), (kind, T)
        assert (passes < N).any() and (passes == N).any(), (kind, T)
        assert [r[0] for r in rounds] == list(range(1, len(rounds) + 1))
        assert [r[2] for r in rounds] == actives, (kind, T)
        assert rounds[-1][3] == st["samples"] == int(passes.sum())
        s1, s2 = _assembled(pref, passes)
        raw, sq, d_passes, rgb_d, err_d = _dev(torch, s1), _dev(torch, s2), _dev(torch, passes), _zeros(torch), _zeros(torch)
        P.film_resolve_counts_device(0, W, H, raw.data_ptr(), d_passes.data_ptr(), rgb_d.data_ptr())
        assert np.array_equal(bits(rgb), bits(rgb_d.cpu().numpy())), (kind, T)
        rel = P.pixel_error_counts_device(0, W, H, d_passes.data_ptr(), raw.data_ptr(), sq.data_ptr(), err_d.data_ptr())
        assert np.array_equal(bits(err), bits(err_d.cpu().numpy())), (kind, T)
        assert np.float64(rounds[-1][4]).view(np.uint64) == np.float64(rel).view(np.uint64)


# ---------------------------------------------------------------- 6. T = 0
@pytest.mark.parametrize("kind", KINDS)
def test_zero_target_is_the_plain_frame(P, scenes, kind):
    _, g = scenes[kind]
    rounds = []
    rgb, err, passes, st = g.render_adaptive(W, H, N, DEPTH[kind], 0.0, min_passes=4, passes_per_round=4,
                                             on_round=lambda *a: rounds.append(a[:4]))
    assert (passes == N).all() and st["samples"] == W * H * N
    assert [r[1] for r in rounds] == [4, 8, 12, 16]
    assert [r[2] for r in rounds] == [W * H, W * H, W * H, 0]
    ref, _ = g.render(W, H, N, DEPTH[kind])
    assert np.array_equal(bits(rgb), bits(ref)), kind


# ---------------------------------------------------------------- 7. exact work
@pytest.mark.parametrize("kind", KINDS)
def test_work_is_exactly_the_sample_set(P, oracle, scenes, prefixes, kind):
    d, g = scenes[kind]
    T = _targets(prefixes[kind], 4, 4, 1e-3)[0]
    rgb, err, passes, st = g.render_adaptive(W, H, N, DEPTH[kind], T, min_passes=4, passes_per_round=4, count_work=True)
    assert st["samples"] == int(passes.sum()) and (passes < N).any()
    ys, xs = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    rep = passes.ravel()
    sx, sy = np.repeat(xs.ravel(), rep), np.repeat(ys.ravel(), rep)
    sp = np.concatenate([np.arange(n) for n in rep])
    _, ct = oracle.Scene(d.ptr, d).trace_samples(W, H, N, DEPTH[kind], sx, sy, sp)
    for k in ("segments", "nodes_tested", "prims_tested", "floor_tested"):
        assert st[k] == ct[k], (kind, k, st[k], ct[k])
    assert ct["samples"] == st["samples"]


# ---------------------------------------------------------------- 8. stopping, determinism, reuse
def test_stop_determinism_and_reuse(P, scenes, prefixes):
    d, g = scenes["cornell"]
    depth = DEPTH["cornell"]
    T = _targets(prefixes["cornell"], 4, 4, 1e-3)[0]
    seen = []

    def stop_at_second(rnd, b, active, samples, rel, im, e, ps):
        seen.append((b, samples, im.copy(), e.copy(), ps.copy()))
        return rnd == 2

    rgb, err, passes, st = g.render_adaptive(W, H, N, depth, T, min_passes=4, passes_per_round=4, on_round=stop_at_second)
    assert len(seen) == 2 and seen[1][0] == 8
    assert np.array_equal(bits(rgb), bits(seen[1][2])) and np.array_equal(bits(err), bits(seen[1][3]))
    assert np.array_equal(passes, seen[1][4]) and passes.max() == 8 and st["samples"] == seen[1][1] == int(passes.sum())
    runs = [g.render_adaptive(W, H, N, depth, T, min_passes=4, passes_per_round=4) for _ in range(2)]
    for a, b in zip(runs[0][:3], runs[1][:3]):
        assert np.array_equal(np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(b).view(np.uint8))

    class Boom(Exception):
        pass

    calls = []

    def boom(rnd, *a):
        calls.append(rnd)
        raise Boom(rnd)

    with pytest.raises(Boom):
        g.render_adaptive(W, H, N, depth, T, min_passes=4, passes_per_round=4, on_round=boom)
    assert calls == [1]
    after, _ = g.render(W, H, N, depth)
    fresh = P.Scene(d.ptr, 0, keepalive=d)
    try:
        want, _ = fresh.render(W, H, N, depth)
    finally:
        fresh.close()
    assert np.array_equal(bits(after), bits(want))


def test_pinned_image_and_the_integrator(P, scenes, prefixes):
    from path_tracer_ocaml_amd import integrator as I
    _, g = scenes["shirley"]
    T = _targets(prefixes["shirley"], 8, 8, 1e-3)[0]
    want, _, want_passes, _ = g.render_adaptive(W, H, N, 8, T)
    img = np.full((H, W, 3), -1.0)
    g.pin_image(img)
    try:
        seen = []
        out, _, passes, _ = g.render_adaptive(W, H, N, 8, T, out=img, on_round=lambda *a: seen.append(a[5] is img))
    finally:
        g.unpin_image()
    assert out is img and seen and all(seen)
    assert np.array_equal(bits(img), bits(want)) and np.array_equal(passes, want_passes)
    image = np.zeros((H, W, 3))
    integ = I.Integrator.create(width=W, height=H, image=image, samples_per_pixel=N, max_bounces=8, scene=g)
    assert integ.render_adaptive(T) is image
    assert np.array_equal(bits(image), bits(want)) and np.array_equal(integ.passes, want_passes)
    assert integ.error.shape == (H, W, 3) and integ.stats["samples"] == int(want_passes.sum())


# ---------------------------------------------------------------- 9. CLI
def test_cli_adaptive(tmp_path):
    exe = os.path.join(ROOT, "path_tracer_ocaml_amd", "shirley_spheres")
    env = dict(os.environ)
    env["LD_LIBRARY_PATH"] = "/opt/rocm/lib:" + env.get("LD_LIBRARY_PATH", "")
    w, h, spp = 200, 100, 32
    base = [exe, f"--dimension={w},{h}", f"--samples-per-pixel={spp}", "--max-ray-bounces=8", "--no-progress"]
    plain, zero = tmp_path / "plain.png", tmp_path / "zero.png"
    r0 = subprocess.run(base + ["-o", str(plain)], capture_output=True, text=True, env=env, timeout=300)
    assert r0.returncode == 0, r0.stderr
    r1 = subprocess.run(base + ["--adaptive=0", "--progressive=4", "-o", str(zero)], capture_output=True, text=True, env=env,
                        timeout=300)
    assert r1.returncode == 0, r1.stderr
    assert zero.read_bytes() == plain.read_bytes()
    pat = re.compile(r"^#round = (\d+), passes = (\d+), active = (\d+), samples = (\d+), error = (\S+)$")
    rounds = [pat.match(l).groups() for l in r1.stdout.splitlines() if l.startswith("#round")]
    assert [int(r[1]) for r in rounds] == list(range(8, spp + 1, 4))
    assert int(rounds[-1][3]) == w * h * spp
    target = float(rounds[0][4])
    r2 = subprocess.run(base + [f"--adaptive={target!r}", "--progressive=4", "--min-passes=4", "-o", str(tmp_path / "a.png")],
                        capture_output=True, text=True, env=env, timeout=300)
    assert r2.returncode == 0, r2.stderr
    rounds = [pat.match(l).groups() for l in r2.stdout.splitlines() if l.startswith("#round")]
    active = [int(r[2]) for r in rounds]
    assert active == sorted(active, reverse=True) and active[0] < w * h
    assert int(rounds[-1][3]) < w * h * spp
    assert any(l.startswith("rendered in: ") for l in r2.stdout.splitlines())
