"""The update machinery of ptx_render_progressive / ptx_render_adaptive / ptx_render_pixels_device / ptx_pixel_error_*_device at
the image sizes where its kernels take another path (tests/test_gpu_adaptive.py and test_gpu_progressive.py run 64 x 48 only:
both sides multiples of 8, 12 workgroups).

  W x H          select entries / blocks / chunk    error blocks   reaches
  1x1 1x40 40x1 7x7   64..320 / 1..2 / 1            1              one ragged tile row or column; up to 63 of 64 lanes off the image
  61 x 37        2560 / 10 / 1                      9              ragged in both axes; last error block partly filled
  256 x 256      65536 / 256 / 1                    256            every scan thread and summary thread used exactly once
  2056 x 32      65792 / 257 / 2                    257            the first size past that: chunk 2, scan threads from 129 on idle
  257 x 257      69696 / 273 / 2                    259            ragged and chunked at once; partial last chunk
  512 x 264      135168 / 528 / 3                   528            chunk 3; the summary's stride loop runs 2 and 3 times

(tests/test_update_reference.py checks this arithmetic.)  The restated rules, the exact summary and its derived bound are
tests/update_reference.py; the scene is Shirley at depth 4 with N = 8, M = 2, K = 3, F = 1e-3: round boundaries 2, 5 and 8.

What the sizes cannot give, said where it is asserted:
* After 2 passes hundreds of Shirley pixels tie at the largest ratio e / d = 1 exactly (one of the two samples is black), so no
  target leaves a ONE-pixel list at 61 x 37 or 257 x 257; a target between the two largest ratios leaves the tied pixels there
  (323 and 9679: no multiple of 64).  The one-pixel list, and the list that keeps every pixel (n_next == npix), run at 40 x 1,
  where the largest ratio is one pixel's and no pixel has zero error.
* 1 x 1 has one pixel and 1 x 40's first target no pixel that stops after 5 passes: LEVELS says which pass counts each target
  leaves, everywhere else all of 2, 5 and 8.
"""
import math

import numpy as np
import pytest

import update_reference as R

pytestmark = pytest.mark.gpu

N, M, K, F, DEPTH = 8, 2, 3, 1e-3, 4
BOUNDS = (2, 5, 8)
SMALL = [(1, 1), (1, 40), (40, 1), (7, 7), (61, 37)]
LARGE = [(256, 256), (2056, 32), (257, 257), (512, 264)]
SIZES = SMALL + LARGE
# the quantiles of the boundary ratios the two targets are taken at; at 512 x 264 the second one is low enough for the second
# round's list to be longer than 65536 entries (asserted), so that a list round goes through the chunked scan as well
QUANTILES = {(512, 264): (0.6, 0.3)}
# the pass counts each of the two targets leaves pixels at, where that is not all three (see the module docstring)
LEVELS = {(1, 40): ({2, 8}, {2, 5, 8})}


def _id(s):
    return f"{s[0]}x{s[1]}"


def bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def same_bits(a, b):
    return np.float64(a).view(np.uint64) == np.float64(b).view(np.uint64)


@pytest.fixture(scope="module")
def P():
    import path_tracer_ocaml_amd as P
    assert P.lib().ptx_device_count() >= 1, P.last_error()
    return P


@pytest.fixture(scope="module")
def torch():
    return pytest.importorskip("torch")


def _zeros(torch, H, W):
    return torch.zeros((H, W, 3), dtype=torch.float64, device="cuda:0")


def _dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


@pytest.fixture(scope="module")
def world(P, torch, oracle):
    """size -> (descriptor, scene on the GPU, {k: (S1, S2)} prefix sums from ptx_render_passes_device in slices), made once"""
    made = {}

    def get(size, at=BOUNDS):
        W, H = size
        if size not in made:
            d = oracle.desc_shirley(W, H)
            made[size] = (d, P.Scene(d.ptr, 0, keepalive=d), {})
        d, g, pref = made[size]
        if not all(k in pref for k in at):
            params = P.render_params(W, H, N, DEPTH)
            raw, sq = _zeros(torch, H, W), _zeros(torch, H, W)
            done = 0
            for k in at:
                g.render_passes_device(params, done, k - done, raw.data_ptr(), sq.data_ptr())
                done = k
                pref.setdefault(k, (raw.cpu().numpy(), sq.cpu().numpy()))
        return d, g, pref

    yield get
    for _, g, _ in made.values():
        g.close()


# ---------------------------------------------------------------- A. the error kernels on synthetic sums
def _sums(rng, npix, k):
    """(S1, S2, same): k non-negative samples per pixel and channel summed in pass order; a tenth of the pixels (`same`) draw k
    equal samples, whose S2 - S1 * S1 / k is zero up to rounding: negative, positive or zero"""
    c = rng.random((k, npix, 3)) * rng.choice([1e-3, 1.0, 40.0], size=(1, npix, 1))
    same = np.zeros(npix, dtype=bool)
    same[rng.permutation(npix)[:npix // 10]] = True
    c[:, same, :] = c[0, same, :]
    s1, s2 = np.zeros((npix, 3)), np.zeros((npix, 3))
    for p in range(k):
        s1, s2 = s1 + c[p], s2 + c[p] * c[p]
    return s1, s2, same


def _within(rel, want, npix):
    return abs(rel - want) <= R.rel_err_bound(npix) * want


@pytest.mark.parametrize("size", SIZES, ids=_id)
def test_error_kernels(P, torch, size):
    W, H = size
    npix = W * H
    nb = R.error_blocks(npix)
    rng = np.random.default_rng(1000 + npix)
    err, err2 = _zeros(torch, H, W), _zeros(torch, H, W)
    for k in (2, 5, 16):
        s1, s2, same = _sums(rng, npix, k)
        v = (s2 - s1 * s1 / k)[same]
        if k >= 3 and same.any():  # (k = 2: all exactly zero; the images under 10 pixels have no such pixel)
            assert (v < 0).any(), (size, k)
        want_se, want_m = R.se(s1, s2, k), R.mean(s1, k)
        want_rel = R.rel_err_exact(want_se, want_m)
        raw, sq = _dev(torch, s1), _dev(torch, s2)
        rel = P.pixel_error_device(0, W, H, k, raw.data_ptr(), sq.data_ptr(), err.data_ptr())
        got = err.cpu().numpy().reshape(npix, 3)
        assert np.array_equal(bits(got), bits(want_se)), (size, k)
        print(f"{_id(size)} k={k}: rel_err off by {(rel - want_rel) / want_rel / R.U:+.2f} u, bound {R.rel_err_bound(npix) / R.U:.0f} u")
        assert _within(rel, want_rel, npix), (size, k, rel, want_rel)
        rel2 = P.pixel_error_device(0, W, H, k, raw.data_ptr(), sq.data_ptr(), err2.data_ptr())
        assert same_bits(rel, rel2) and torch.equal(err.view(torch.int64), err2.view(torch.int64)), (size, k)
        err2.zero_()
        uniform = _dev(torch, np.full((H, W), k, dtype=np.int32))
        rel3 = P.pixel_error_counts_device(0, W, H, uniform.data_ptr(), raw.data_ptr(), sq.data_ptr(), err2.data_ptr())
        assert same_bits(rel, rel3) and torch.equal(err.view(torch.int64), err2.view(torch.int64)), (size, k)
    # a non-uniform count map, k in 2 .. 16, over the last sums
    m = rng.integers(2, 17, npix).astype(np.int32)
    want_se, want_m = R.se(s1, s2, m), R.mean(s1, m)
    d_m = _dev(torch, m)
    rel = P.pixel_error_counts_device(0, W, H, d_m.data_ptr(), raw.data_ptr(), sq.data_ptr(), err.data_ptr())
    assert np.array_equal(bits(err.cpu().numpy().reshape(npix, 3)), bits(want_se)), size
    assert _within(rel, R.rel_err_exact(want_se, want_m), npix), size
    # one pixel with a single pass in the last (partly filled) block: +inf there and in the summary
    m1 = m.copy()
    m1[npix - 1] = 1
    d_m1 = _dev(torch, m1)
    assert P.pixel_error_counts_device(0, W, H, d_m1.data_ptr(), raw.data_ptr(), sq.data_ptr(), err.data_ptr()) == math.inf
    got = err.cpu().numpy().reshape(npix, 3)
    assert np.isinf(got[npix - 1]).all() and (got[npix - 1] > 0).all() and np.array_equal(bits(got[:-1]), bits(want_se[:-1]))
    # all zero: 0, and a zero error image
    z = _zeros(torch, H, W)
    err.fill_(-1.0)
    assert P.pixel_error_device(0, W, H, 5, z.data_ptr(), z.data_ptr(), err.data_ptr()) == 0.0
    assert float(err.abs().max()) == 0.0
    assert P.pixel_error_counts_device(0, W, H, d_m.data_ptr(), z.data_ptr(), z.data_ptr()) == 0.0
    # block weight: everything zero but one pixel, in error block j, on its first lane and on its last: rel_err is that pixel's
    # own, whatever block it sits in.  A reduction that drops or double-counts a block (or half of one) fails here.
    one1, one2 = np.array([3.0, 0.5, 7.0]), np.array([2.5, 0.0625, 11.0])
    own = R.rel_err_exact(R.se(one1, one2, 5), R.mean(one1, 5))
    assert 0.0 < own < math.inf
    z2 = _zeros(torch, H, W)
    f1, f2 = z.view(-1, 3), z2.view(-1, 3)
    d1, d2 = _dev(torch, one1), _dev(torch, one2)
    blocks = sorted({j for j in (0, 1, 255, 256, 257, nb - 2, nb - 1) if 0 <= j < nb})
    for j in blocks:
        for p in sorted({j * 256, min(j * 256 + 255, npix - 1)}):
            f1[p], f2[p] = d1, d2
            rel = P.pixel_error_device(0, W, H, 5, z.data_ptr(), z2.data_ptr())
            relc = P.pixel_error_counts_device(0, W, H, uniform.data_ptr(), z.data_ptr(), z2.data_ptr()) if j == nb - 1 else rel
            f1[p], f2[p] = 0.0, 0.0
            assert _within(rel, own, npix), (size, j, p, rel, own)
            assert j != nb - 1 or _within(relc, R.rel_err_exact(R.se(one1, one2, 16), R.mean(one1, 16)), npix), (size, j, p)


# ---------------------------------------------------------------- B. adaptive rounds
def _anchor(oracle, d, pref, W, H):
    """the prefix sums are the oracle's per-sample radiance summed in pass order, bit for bit: at every pixel of a small image,
    at a seeded sample of 2000 plus the corners, the last row and the last column of a large one"""
    npix = W * H
    if (W, H) in SMALL:
        pix = np.arange(npix)
    else:
        rng = np.random.default_rng(npix)
        edge = np.concatenate([(H - 1) * W + np.arange(W), np.arange(H) * W + (W - 1), [0, W - 1, (H - 1) * W, npix - 1]])
        pix = np.unique(np.concatenate([rng.choice(npix, 2000, replace=False), edge]))
    xs, ys = np.repeat(pix % W, N), np.repeat(pix // W, N)
    rgb, _ = oracle.Scene(d.ptr, d).trace_samples(W, H, N, DEPTH, xs, ys, np.tile(np.arange(N), len(pix)))
    per = rgb.reshape(len(pix), N, 3)
    s1, s2 = np.zeros((len(pix), 3)), np.zeros((len(pix), 3))
    for k in range(N):
        s1, s2 = s1 + per[:, k], s2 + per[:, k] * per[:, k]
        if k + 1 in pref:
            g1, g2 = pref[k + 1][0].reshape(npix, 3)[pix], pref[k + 1][1].reshape(npix, 3)[pix]
            assert np.array_equal(bits(s1), bits(g1)) and np.array_equal(bits(s2), bits(g2)), ((W, H), k + 1)
    assert float(s1.max()) > 0.0


def _run_and_check(P, torch, g, pref, W, H, T):
    """one ptx_render_adaptive run against the restatement: the pass map, the active counts, the samples, the film and the error
    of the assembled prefixes.  A lost pixel shows in the map, a duplicated one (two adds of the same samples) in the sums."""
    want, actives = R.restate_rounds(pref, W, H, N, M, K, T, F)
    rounds = []
    rgb, err, passes, st = g.render_adaptive(W, H, N, DEPTH, T, min_passes=M, passes_per_round=K, radiance_floor=F,
                                             on_round=lambda *a: rounds.append(a[:5]))
    assert np.array_equal(passes, want), ((W, H), T, int((passes != want).sum()))
    assert [r[0] for r in rounds] == list(range(1, len(rounds) + 1))
    assert [r[2] for r in rounds] == actives, ((W, H), T)
    assert rounds[-1][3] == st["samples"] == int(passes.sum())
    s1, s2 = R.assembled(pref, passes)
    raw, sq, d_passes, rgb_d, err_d = _dev(torch, s1), _dev(torch, s2), _dev(torch, passes), _zeros(torch, H, W), _zeros(torch, H, W)
    P.film_resolve_counts_device(0, W, H, raw.data_ptr(), d_passes.data_ptr(), rgb_d.data_ptr())
    assert np.array_equal(bits(rgb), bits(rgb_d.cpu().numpy())), ((W, H), T)
    rel = P.pixel_error_counts_device(0, W, H, d_passes.data_ptr(), raw.data_ptr(), sq.data_ptr(), err_d.data_ptr())
    assert np.array_equal(bits(err), bits(err_d.cpu().numpy())), ((W, H), T)
    assert same_bits(rounds[-1][4], rel)
    return passes, actives, rounds, (rgb, err)


@pytest.mark.parametrize("size", SIZES, ids=_id)
def test_adaptive_rounds(P, torch, oracle, world, size):
    W, H = size
    npix = W * H
    d, g, pref = world(size)
    _anchor(oracle, d, pref, W, H)
    if size == (1, 1):
        # one pixel: no target leaves pixels at three pass counts.  Below, between and above its two ratios: it runs to N,
        # stops where the restatement says, and stops after M
        r = sorted(float(q[0, 0]) for _, q in R.boundary_ratios(pref, N, M, K, F))
        assert 0.0 < r[0] < r[1]
        seen = [int(_run_and_check(P, torch, g, pref, W, H, T)[0][0, 0]) for T in (0.5 * r[0], 0.5 * (r[0] + r[1]), 2.0 * r[1])]
        assert seen[0] == N and seen[2] == M and seen[1] in BOUNDS
        return
    for T, levels in zip(R.targets(pref, N, M, K, F, QUANTILES.get(size, (0.35, 0.6))), LEVELS.get(size, ({2, 5, 8},) * 2)):
        passes, actives, _, _ = _run_and_check(P, torch, g, pref, W, H, T)
        assert set(np.unique(passes).tolist()) == levels, (size, T)
        assert 0 < actives[0] < npix
    if size == (512, 264):
        assert actives[0] > 65536  # the second round's list: its select has 257+ workgroups, with pix != nullptr


EDGES = {(40, 1): dict(top=1, all_stay=True), (61, 37): dict(top=323, all_stay=False), (257, 257): dict(top=9679, all_stay=False)}


@pytest.mark.parametrize("size", list(EDGES), ids=_id)
def test_list_edges(P, torch, world, size):
    W, H = size
    npix = W * H
    _, g, pref = world(size)
    q2 = R.boundary_ratios(pref, N, M, K, F)[0][1]
    u = np.unique(q2)
    # between the two largest ratios after M passes: the next list holds the pixels at the largest (one, where it is not tied)
    T = 0.5 * (u[-1] + u[-2])
    assert u[-1] - T >= 1e-6 * T and T - u[-2] >= 1e-6 * T
    _, actives, _, _ = _run_and_check(P, torch, g, pref, W, H, T)
    assert actives[0] == int((q2 == u[-1]).sum()) == EDGES[size]["top"], actives
    assert actives[0] % 64 != 0
    # below the smallest positive ratio of every boundary: every pixel with a non-zero error stays, to the end
    pos = np.concatenate([q[q > 0] for _, q in R.boundary_ratios(pref, N, M, K, F)])
    passes, actives, _, _ = _run_and_check(P, torch, g, pref, W, H, 0.5 * float(pos.min()))
    assert actives[0] == int((q2 > 0).sum()) and actives[0] % 256 != 0
    assert (actives[0] == npix) == EDGES[size]["all_stay"], actives  # n_next == npix: the round is a plain slice again
    # everything converges: one round
    passes, actives, rounds, _ = _run_and_check(P, torch, g, pref, W, H, 1e30)
    assert (passes == M).all() and actives == [0] and len(rounds) == 1 and rounds[0][1] == M and rounds[0][3] == npix * M
    # T = 0: no select at all, the plain frame
    rounds = []
    rgb, err, passes, st = g.render_adaptive(W, H, N, DEPTH, 0.0, min_passes=M, passes_per_round=K, radiance_floor=F,
                                             on_round=lambda *a: rounds.append(a[:4]))
    assert (passes == N).all() and st["samples"] == npix * N
    assert [r[1] for r in rounds] == [2, 5, 8] and [r[2] for r in rounds] == [npix, npix, 0]
    ref, _ = g.render(W, H, N, DEPTH)
    assert np.array_equal(bits(rgb), bits(ref)), size


def test_two_runs_give_the_same_bytes(P, torch, world):
    W, H = 257, 257
    _, g, pref = world((W, H))
    T = R.targets(pref, N, M, K, F)[0]
    runs = [g.render_adaptive(W, H, N, DEPTH, T, min_passes=M, passes_per_round=K, radiance_floor=F) for _ in range(2)]
    for a, b in zip(runs[0][:3], runs[1][:3]):
        assert np.array_equal(np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(b).view(np.uint8))
    assert (runs[0][2] < N).any() and (runs[0][2] == N).any()


# ---------------------------------------------------------------- C. pixel lists at their edges
@pytest.mark.parametrize("size", [(61, 37), (257, 257)], ids=_id)
def test_pixel_lists(P, torch, world, size):
    W, H = size
    npix = W * H
    _, g, pref = world(size)
    ref1, ref2 = pref[N][0].reshape(npix, 3), pref[N][1].reshape(npix, 3)
    rng = np.random.default_rng(npix)
    lists = {"last": np.array([npix - 1]), "r63": rng.choice(npix, 63, replace=False), "r257": rng.choice(npix, 257, replace=False),
             "reversed": np.arange(npix)[::-1].copy()}
    if npix > 65537:
        lists["r65537"] = rng.choice(npix, 65537, replace=False)
    params = P.render_params(W, H, N, DEPTH)
    for name, lst in lists.items():
        raw, sq = _zeros(torch, H, W), _zeros(torch, H, W)
        d_list = _dev(torch, lst.astype(np.int32))
        for a, c in ((0, 3), (3, 1), (4, 4)):
            st = g.render_pixels_device(params, a, c, d_list.data_ptr(), len(lst), raw.data_ptr(), sq.data_ptr())
            assert st["samples"] == len(lst) * c, (size, name)
        got1, got2 = raw.cpu().numpy().reshape(npix, 3), sq.cpu().numpy().reshape(npix, 3)
        assert np.array_equal(bits(got1[lst]), bits(ref1[lst])) and np.array_equal(bits(got2[lst]), bits(ref2[lst])), (size, name)
        off = np.ones(npix, dtype=bool)
        off[lst] = False
        assert (got1[off] == 0.0).all() and (got2[off] == 0.0).all(), (size, name)
    assert float(ref1[npix - 1].max()) > 0.0


# ---------------------------------------------------------------- D. progressive updates
@pytest.mark.parametrize("size", [(61, 37), (2056, 32), (257, 257)], ids=_id)
def test_progressive_updates(P, torch, world, size):
    W, H = size
    npix = W * H
    _, g, pref = world(size, at=(3, 6, 8))
    seen = []
    rgb, err, done, st = g.render_progressive(W, H, N, DEPTH, 3, on_update=lambda k, rel, im, e: seen.append((k, rel, im.copy(), e.copy())))
    assert [s[0] for s in seen] == [3, 6, 8] and done == N and st["samples"] == npix * N
    rgb_d, err_d = _zeros(torch, H, W), _zeros(torch, H, W)
    for k, rel, im, e in seen:
        s1, s2 = pref[k]
        raw, sq = _dev(torch, s1), _dev(torch, s2)
        P.film_resolve_device(0, W, H, k, raw.data_ptr(), rgb_d.data_ptr())
        assert np.array_equal(bits(im), bits(rgb_d.cpu().numpy())), (size, k)
        want_rel = P.pixel_error_device(0, W, H, k, raw.data_ptr(), sq.data_ptr(), err_d.data_ptr())
        assert same_bits(rel, want_rel) and np.array_equal(bits(e), bits(err_d.cpu().numpy())), (size, k)
        exact = R.rel_err_exact(R.se(s1, s2, k), R.mean(s1, k))
        assert 0.0 < exact < math.inf and _within(rel, exact, npix), (size, k, rel, exact)
    assert np.array_equal(bits(rgb), bits(seen[-1][2])) and np.array_equal(bits(err), bits(seen[-1][3]))
    target = seen[1][1]
    assert seen[0][1] > target
    _, _, done, st = g.render_progressive(W, H, N, DEPTH, 3, target_rel_err=target)
    assert done == 6 and st["samples"] == npix * 6
