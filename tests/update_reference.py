"""The rules behind the progressive and adaptive updates, restated once in numpy for any (W, H, N).

* se: the per-channel standard error of include/ptx.h (ptx_pixel_error_device), operation for operation in binary64 -- every
  step is one correctly rounded IEEE operation on the device too (the build has contraction off), so the device's err equals it
  bit for bit.
* ratio / restate_rounds / targets / assembled: the stopping rule of ptx_render_adaptive and the rounds it implies, from the
  pass-order prefix sums {k: (S1, S2)} at the round boundaries.
* rel_err_exact / rel_err_bound: the frame summary with exactly rounded sums, and how far a fixed-order binary64 reduction of
  the same terms may lie from it.
* tile_order: the whole image in pt_primary_decode's 8x8-tile order, the order the adaptive select keeps.
"""
import math

import numpy as np

U = 2.0 ** -53  # unit roundoff of binary64


def _per_pixel(k, like):
    """k (a number, or one count per pixel) shaped to broadcast against the (..., 3) sums"""
    k = np.asarray(k, dtype=np.float64)
    return k[..., None] if k.ndim == np.ndim(like) - 1 and k.ndim > 0 else k


def se(s1, s2, k):
    """sqrt(max(0, S2 - S1 * S1 / k) / (k (k - 1))) for k >= 2, +inf below; k a number or an array of per-pixel counts"""
    s1, s2 = np.asarray(s1, dtype=np.float64), np.asarray(s2, dtype=np.float64)
    kd = _per_pixel(k, s1)
    with np.errstate(divide="ignore", invalid="ignore"):
        v = s2 - s1 * s1 / kd
        out = np.sqrt(np.where(v > 0.0, v, 0.0) / (kd * (kd - 1.0)))
    return np.where(kd >= 2.0, out, np.inf)


def mean(s1, k):
    s1 = np.asarray(s1, dtype=np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        return s1 / _per_pixel(k, s1)


def ratio(s1, s2, k):
    """(e, d0) of the stopping rule after k passes: e = sqrt((se_r^2 + se_g^2) + se_b^2), d0 = sqrt((m_r^2 + m_g^2) + m_b^2);
    a pixel has converged when T > 0 and e <= T * max(d0, F)"""
    kd = float(k)
    s = np.sqrt(np.maximum(0.0, s2 - s1 * s1 / kd) / (kd * (kd - 1.0)))
    m = s1 / kd
    e = np.sqrt((s[..., 0] * s[..., 0] + s[..., 1] * s[..., 1]) + s[..., 2] * s[..., 2])
    d = np.sqrt((m[..., 0] * m[..., 0] + m[..., 1] * m[..., 1]) + m[..., 2] * m[..., 2])
    return e, d


def boundaries(N, M, K):
    """the pass counts after which a round may be followed by another: min(M, N), then every K up to (not including) N"""
    return list(range(min(M, N), N, K))


def restate_rounds(prefixes, W, H, N, M, K, T, F):
    """the pass map the rounds give, and each round's count of pixels for the next round"""
    b = min(M, N)
    passes = np.full((H, W), b, dtype=np.int32)
    active = np.ones((H, W), dtype=bool)
    actives = []
    while b < N:
        e, d = ratio(*prefixes[b], b)
        if T > 0:
            active &= ~(e <= T * np.maximum(d, F))
        actives.append(int(active.sum()))
        if not active.any():
            return passes, actives
        b = min(b + K, N)
        passes[active] = b
    actives.append(0)
    return passes, actives


def boundary_ratios(prefixes, N, M, K, F):
    """e / max(d0, F) of every pixel at every round boundary: [(b, (H, W) array)]"""
    out = []
    for b in boundaries(N, M, K):
        e, d = ratio(*prefixes[b], b)
        out.append((b, e / np.maximum(d, F)))
    return out


def clear_target(r, i, margin=1e-6):
    """the midpoint of two neighbouring values of the sorted ratios r, from index i upwards, that lies at least `margin`
    relative from every one of them: no pixel is near enough to the threshold for the last bit of e or d to decide it"""
    while True:
        t = 0.5 * (r[i] + r[i + 1])
        if np.abs(r - t).min() >= margin * t:
            return t
        i += 1


def targets(prefixes, N, M, K, F, quantiles=(0.35, 0.6)):
    """targets at least 1e-6 relative from every pixel's e / d at every round boundary, one per quantile of those ratios"""
    r = np.unique(np.concatenate([q.ravel() for _, q in boundary_ratios(prefixes, N, M, K, F)]))
    r = r[np.isfinite(r) & (r > 0)]
    return [clear_target(r, int(q * len(r))) for q in quantiles]


def assembled(prefixes, passes):
    """the sums a pixel that stopped after passes[y, x] passes holds: its own prefix at that count"""
    s1, s2 = np.zeros(passes.shape + (3,)), np.zeros(passes.shape + (3,))
    for k in np.unique(passes):
        at = passes == k
        s1[at], s2[at] = prefixes[int(k)][0][at], prefixes[int(k)][1][at]
    return s1, s2


def rel_err_exact(se_, mean_):
    """sqrt(sum se^2) / sqrt(sum mean^2) with the products in binary64 (the device's addends) and both sums exactly rounded
    (math.fsum); 0 when both sums are 0, +inf when any se is infinite (a pixel with k < 2)"""
    s = np.asarray(se_, dtype=np.float64).ravel()
    m = np.asarray(mean_, dtype=np.float64).ravel()
    if np.isinf(s).any():
        return math.inf
    a, b = math.fsum((s * s).tolist()), math.fsum((m * m).tolist())
    if a == 0.0 and b == 0.0:
        return 0.0
    return math.sqrt(a) / math.sqrt(b) if b > 0.0 else math.inf


def error_blocks(npix):
    return (npix + 255) // 256


def rel_err_bound(npix):
    """How far, relative, the device's rel_err may lie from rel_err_exact.

    Both sums have non-negative addends (se^2 and mean^2, the same binary64 products on both sides), so no addition cancels
    and a sum that passes every term through at most d additions, each rounded once, is within (1 + u)^d - 1 ~ d u of the
    exact sum, u = 2^-53.  The longest chain a term passes through on the device:
      3   the pixel's channels, added in turn to a zero (k_pixel_error),
      8   the tree over the 256 threads of a block (pt_error_block_sum),
      ceil(ceil(npix / 256) / 256)   a summary thread's stride loop over the blocks t, t + 256, ... (k_error_summary),
      8   the summary's tree.
    A square root halves a relative error and adds one rounding; the division adds one.  Both sums err by at most d u, so the
    quotient of the roots errs by at most d u from the sums plus three roundings; one more u covers the second-order terms
    and the reference's own last step.  Hence (d + 4) u: 26 * 2^-53 at 512 x 264."""
    d = 3 + 8 + -(-error_blocks(npix) // 256) + 8
    return (d + 4) * U


def tile_order(W, H):
    """the pixel indices y * W + x of the whole image in pt_primary_decode's order: 8x8 tiles row by row, inside a tile lane
    l = 8 (y % 8) + (x % 8); lanes off the image left out"""
    tiles_x, tiles_y = (W + 7) // 8, (H + 7) // 8
    lane = np.arange(64)
    tile = np.arange(tiles_x * tiles_y)
    x = (tile % tiles_x)[:, None] * 8 + (lane & 7)[None, :]
    y = (tile // tiles_x)[:, None] * 8 + (lane >> 3)[None, :]
    on = (x < W) & (y < H)
    return (y * W + x)[on].astype(np.int64)


def select_blocks(W, H):
    """(entries, workgroups, chunk) of the whole-image select: AdaptivePolicy::padded(), its 256-entry blocks, and the blocks one
    thread of k_select_scan scans"""
    padded = ((W + 7) // 8) * ((H + 7) // 8) * 64
    nb = (padded + 255) // 256
    return padded, nb, -(-nb // 256)
