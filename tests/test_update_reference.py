"""tests/update_reference.py against what it restates: exact arithmetic for the summary, pass maps known by construction for the
rounds, a permutation for the tile order.  No GPU."""
import math

import numpy as np
import pytest

import update_reference as R

# the sizes of tests/test_gpu_update_sizes.py
SIZES = [(1, 1), (1, 40), (40, 1), (7, 7), (61, 37), (256, 256), (2056, 32), (257, 257), (512, 264)]


def _random_sums(rng, npix, k):
    """(S1, S2) of k non-negative samples per pixel and channel, summed in pass order"""
    c = rng.random((k, npix, 3)) * rng.choice([1e-3, 1.0, 50.0], size=(1, npix, 1))
    s1, s2 = np.zeros((npix, 3)), np.zeros((npix, 3))
    for p in range(k):
        s1, s2 = s1 + c[p], s2 + c[p] * c[p]
    return s1, s2


def test_se_is_the_documented_formula():
    s1, s2 = np.array([[3.0, 0.0, 2.0]]), np.array([[5.0, 0.0, 1.0]])
    got = R.se(s1, s2, 2)
    # k = 2: (5 - 9/2) / 2 = 0.25 -> 0.5; zero sums -> 0; 1 - 4/2 < 0 -> clamped to 0
    assert got.tolist() == [[0.5, 0.0, 0.0]]
    assert np.isinf(R.se(s1, s2, 1)).all() and (R.se(s1, s2, 1) > 0).all()
    k = np.array([1, 2, 4])
    per = R.se(np.tile(s1, (3, 1)), np.tile(s2, (3, 1)), k)
    assert np.isinf(per[0]).all() and per[1].tolist() == [0.5, 0.0, 0.0]
    assert per[2, 0] == math.sqrt((5.0 - 9.0 / 4.0) / 12.0)
    assert np.array_equal(R.mean(np.tile(s1, (3, 1)), k), np.tile(s1, (3, 1)) / k[:, None])


def test_rel_err_exact_against_60_digits():
    import mpmath as mp
    rng = np.random.default_rng(21)
    with mp.workdps(60):
        for n in (1, 2, 3, 17, 256, 257, 4099):
            for k in (2, 5, 16):
                s1, s2 = _random_sums(rng, n, k)
                s, m = R.se(s1, s2, k), R.mean(s1, k)
                a = mp.fsum(mp.mpf(float(v)) for v in (s * s).ravel())
                b = mp.fsum(mp.mpf(float(v)) for v in (m * m).ravel())
                want = mp.sqrt(a) / mp.sqrt(b)
                got = R.rel_err_exact(s, m)
                assert abs(mp.mpf(got) - want) <= 2 * R.U * want, (n, k, got)
    assert R.rel_err_exact(np.zeros((5, 3)), np.zeros((5, 3))) == 0.0
    one = np.zeros((5, 3))
    one[4, 2] = np.inf
    assert R.rel_err_exact(one, np.ones((5, 3))) == math.inf


def test_rel_err_bound_is_the_derived_figure():
    assert R.rel_err_bound(512 * 264) == 26 * 2.0 ** -53
    assert R.rel_err_bound(1) == 24 * 2.0 ** -53 == R.rel_err_bound(256 * 256)
    assert R.rel_err_bound(256 * 256 + 1) == 25 * 2.0 ** -53 == R.rel_err_bound(257 * 257)


def _tree(x):
    """pt_error_block_sum over the last axis (256 wide): off = 128, 64, ..., 1"""
    x = x.copy()
    off = 128
    while off > 0:
        x[..., :off] = x[..., :off] + x[..., off:2 * off]
        off >>= 1
    return x[..., 0]


def device_order_sum(terms):
    """the (npix, 3) non-negative terms added as k_pixel_error and k_error_summary add them, in plain binary64"""
    npix = terms.shape[0]
    per = ((0.0 + terms[:, 0]) + terms[:, 1]) + terms[:, 2]
    nb = R.error_blocks(npix)
    padded = np.zeros(nb * 256)
    padded[:npix] = per
    partial = _tree(padded.reshape(nb, 256))
    acc = np.zeros(256)
    for first in range(0, nb, 256):  # thread t adds blocks t, t + 256, ... in turn
        part = partial[first:first + 256]
        acc[:len(part)] = acc[:len(part)] + part
    return float(_tree(acc))


@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_a_fixed_order_sum_meets_the_bound(size):
    W, H = size
    npix = W * H
    rng = np.random.default_rng(npix)
    for k in (2, 5, 16):
        s1, s2 = _random_sums(rng, npix, k)
        s, m = R.se(s1, s2, k), R.mean(s1, k)
        a, b = device_order_sum(s * s), device_order_sum(m * m)
        got = math.sqrt(a) / math.sqrt(b)
        want = R.rel_err_exact(s, m)
        assert abs(got - want) <= R.rel_err_bound(npix) * want, (size, k, (got - want) / want / R.U)
    # the plain sum is the exact one where every addition is exact
    ones = np.ones((npix, 3))
    assert device_order_sum(ones) == 3.0 * npix


# ---------------------------------------------------------------- the rounds on a table whose pass map is known
N, M, K, F, T = 8, 2, 3, 1e-3, 0.05
STEADY = [1.0] * 8                                  # se = 0 at every boundary: stops after M = 2
NOISY = [0.0, 2.0] * 4                              # se / mean >= 1 / sqrt(8): never stops
LATE = [0.9, 1.1, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0]     # ratio 0.1 after 2 passes, 0.0316 after 5: stops after 5


def _table(kinds):
    """{k: (S1, S2)} for an image whose pixel (y, x) draws the sample sequence kinds[y][x] on all three channels"""
    H, W = len(kinds), len(kinds[0])
    c = np.array([[kinds[y][x] for x in range(W)] for y in range(H)], dtype=np.float64)  # (H, W, N)
    out = {}
    s1, s2 = np.zeros((H, W, 3)), np.zeros((H, W, 3))
    for p in range(N):
        s1, s2 = s1 + c[:, :, p, None], s2 + (c[:, :, p] * c[:, :, p])[..., None]
        out[p + 1] = (s1, s2)
    return out, W, H


def test_restated_rounds_on_known_maps():
    assert R.boundaries(N, M, K) == [2, 5]
    W, H = 5, 4
    grid = lambda f: [[f(x, y) for x in range(W)] for y in range(H)]  # noqa: E731
    # everything converges after the first round
    pref, _, _ = _table(grid(lambda x, y: STEADY))
    passes, actives = R.restate_rounds(pref, W, H, N, M, K, T, F)
    assert (passes == 2).all() and actives == [0]
    # nothing converges
    pref, _, _ = _table(grid(lambda x, y: NOISY))
    passes, actives = R.restate_rounds(pref, W, H, N, M, K, T, F)
    assert (passes == 8).all() and actives == [20, 20, 0]
    # T = 0: nothing converges whatever the samples are
    pref, _, _ = _table(grid(lambda x, y: STEADY))
    passes, actives = R.restate_rounds(pref, W, H, N, M, K, 0.0, F)
    assert (passes == 8).all() and actives == [20, 20, 0]
    # one pixel goes on, to the end; one that stops after the second round
    for seq, n, want_act in ((NOISY, 8, [1, 1, 0]), (LATE, 5, [1, 0])):
        pref, _, _ = _table(grid(lambda x, y: seq if (x, y) == (3, 2) else STEADY))
        passes, actives = R.restate_rounds(pref, W, H, N, M, K, T, F)
        want = np.full((H, W), 2)
        want[2, 3] = n
        assert np.array_equal(passes, want) and actives == want_act, seq
    # a checkerboard of the three kinds
    kinds = grid(lambda x, y: (STEADY, NOISY, LATE)[(x + y) % 3])
    pref, _, _ = _table(kinds)
    passes, actives = R.restate_rounds(pref, W, H, N, M, K, T, F)
    want = np.array([[(2, 8, 5)[(x + y) % 3] for x in range(W)] for y in range(H)])
    assert np.array_equal(passes, want)
    assert actives == [int((want > 2).sum()), int((want > 5).sum()), 0]
    s1, s2 = R.assembled(pref, passes)
    for (y, x), n in np.ndenumerate(want):
        assert np.array_equal(s1[y, x], pref[n][0][y, x]) and np.array_equal(s2[y, x], pref[n][1][y, x])
    # the floor: a dark pixel is measured against F, not against its own mean
    dark = [v * 1e-6 for v in NOISY]
    pref, _, _ = _table(grid(lambda x, y: dark))
    assert (R.restate_rounds(pref, W, H, N, M, K, T, F)[0] == 2).all()
    assert (R.restate_rounds(pref, W, H, N, M, K, T, 0.0)[0] == 8).all()
    # the finder's targets keep clear of every ratio
    pref, _, _ = _table(kinds)
    r = np.concatenate([q.ravel() for _, q in R.boundary_ratios(pref, N, M, K, F)])
    for t in R.targets(pref, N, M, K, F, quantiles=(0.0, 0.5)):
        assert (np.abs(r - t) >= 1e-6 * t).all() and r.min() < t < r.max()


@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_tile_order_is_a_permutation(size):
    W, H = size
    order = R.tile_order(W, H)
    assert order.dtype == np.int64 and np.array_equal(np.sort(order), np.arange(W * H))
    # tile by tile, rows of 8 inside a tile: a restatement by loops on the sizes where that is cheap
    if W * H <= 4096:
        want = []
        for ty in range((H + 7) // 8):
            for tx in range((W + 7) // 8):
                for lane in range(64):
                    x, y = tx * 8 + (lane & 7), ty * 8 + (lane >> 3)
                    if x < W and y < H:
                        want.append(y * W + x)
        assert order.tolist() == want
    padded, nb, chunk = R.select_blocks(W, H)
    assert padded >= W * H and nb == -(-padded // 256) and chunk == -(-nb // 256)


def test_the_sizes_reach_what_they_are_for():
    """the block arithmetic of AdaptivePolicy::queue_update and pixel_error_blocks at the GPU file's sizes"""
    got = {s: R.select_blocks(*s) + (R.error_blocks(s[0] * s[1]),) for s in SIZES}
    assert got[(1, 1)] == (64, 1, 1, 1) and got[(40, 1)] == (320, 2, 1, 1) and got[(7, 7)] == (64, 1, 1, 1)
    assert got[(61, 37)] == (2560, 10, 1, 9)
    assert got[(256, 256)] == (65536, 256, 1, 256)
    assert got[(2056, 32)] == (65792, 257, 2, 257)
    assert got[(257, 257)] == (69696, 273, 2, 259)
    assert got[(512, 264)] == (135168, 528, 3, 528)
