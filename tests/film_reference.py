"""The film at any order and radius, restated for the tests (not a test itself): Binomial.create's weights in fractions.Fraction,
the gather rule of include/ptx.h with an exact fma, the banded row map, the counts rule, and Film_tile.write_pixel + stitch_tile as
a splat for one tile that is the whole image.

Every operation is binary64 as the rule writes it: Python's float +, *, / and math.sqrt are correctly rounded, and the fma is
float(Fraction(a) * Fraction(b) + Fraction(c)) -- here without the reduction to lowest terms: the sum over the common power-of-two
denominator, one correctly rounded integer division at the end (fma_exact is the literal form, tests compare the two)."""
import math
from fractions import Fraction

import numpy as np

RENORMALISE = 1
MAX_ORDER, MAX_RADIUS = 16, 7


def accepted_pairs():
    """the 72 (order, radius) the library accepts"""
    return [(o, r) for o in range(1, MAX_ORDER + 1) for r in range(0, MAX_RADIUS + 1) if o >= 2 * r + 1]


def weights_raw(order, radius):
    """filter_kernel.ml:49-85 up to float_of_num: tap i of the 2r + 1 covers [i * ratio, (i + 1) * ratio) of the binomial row of
    `order` coefficients; the first covered cell weighs one minus the fractional part of the tap's start, else the last one minus
    what it sticks out beyond the tap's end, every other cell one.  Exact rationals."""
    f_width = 1 + 2 * radius
    ratio = Fraction(order, f_width)
    coeffs = [math.comb(order - 1, k) for k in range(order)]
    out = []
    for i in range(f_width):
        lo = i * ratio
        hi = lo + ratio
        beg = math.floor(lo)
        end = math.ceil(hi)
        n = end - beg
        total = Fraction(0)
        for k in range(n):
            if k == 0:
                wk = 1 - (lo - math.floor(lo))
            elif k == n - 1:
                wk = 1 - (end - hi)
            else:
                wk = Fraction(1)
            total += wk * coeffs[k + beg]
        out.append(total)
    return out


def weights(order, radius):
    """(w1d, w2d) as lists of floats: float_of_num to nearest, the left fold of + from 0.0, w / total, then w[j] * w[i]"""
    w = [float(q) for q in weights_raw(order, radius)]  # float(Fraction) rounds to nearest
    total = 0.0
    for v in w:
        total = total + v
    w = [v / total for v in w]
    return w, [[wj * wi for wi in w] for wj in w]


def fma_exact(a, b, c):
    return float(Fraction(a) * Fraction(b) + Fraction(c))


def fma(a, b, c):
    """fma_exact for finite operands: int / int is correctly rounded"""
    na, da = a.as_integer_ratio()
    nb, db = b.as_integer_ratio()
    nc, dc = c.as_integer_ratio()
    dab = da * db
    return (na * nb * dc + nc * dab) / (dab * dc)


def band_row_index(y, world, band_rows, pad_rows):
    """row of the gathered [world * pad_rows] buffer that holds image row y"""
    if world <= 1:
        return y
    band = y // band_rows
    rank = band % world
    local = (band // world) * band_rows + (y - band * band_rows)
    return rank * pad_rows + local


def local_rows(height, world, band_rows, rank):
    n_bands = (height + band_rows - 1) // band_rows
    return sum(min((b + 1) * band_rows, height) - b * band_rows for b in range(rank, n_bands, world))


def to_banded(S, world, band_rows, extra_pad=1, fill=float("nan")):
    """(gathered [world, pad_rows, W, 3], pad_rows): the image's rows dealt to the ranks band by band; the rows no image row
    lands on hold `fill`"""
    H, W, _ = S.shape
    pad_rows = max(local_rows(H, world, band_rows, k) for k in range(world)) + extra_pad
    g = np.full((world * pad_rows, W, 3), fill)
    for y in range(H):
        g[band_row_index(y, world, band_rows, pad_rows)] = S[y]
    return g.reshape(world, pad_rows, W, 3), pad_rows


def accumulate(S, order, radius, counts=None):
    """The rule's loop for every pixel of S (H, W, 3): (acc (H, W, 3), ws (H, W), clipped (H, W), same (H, W)).  Without counts every
    pixel is `same`; with them a pixel whose in-image window holds another count accumulates each tap's own mean S(q) * (1.0 / n(q))."""
    H, W, _ = S.shape
    w, _ = weights(order, radius)
    r = radius
    acc = np.zeros((H, W, 3))
    ws = np.zeros((H, W))
    clipped = np.zeros((H, W), dtype=bool)
    same = np.ones((H, W), dtype=bool)
    Sl = S.tolist()
    for y in range(H):
        for x in range(W):
            taps = []
            for dy in range(-r, r + 1):
                for dx in range(-r, r + 1):
                    sx, sy = x - dx, y - dy
                    if sx < 0 or sx >= W or sy < 0 or sy >= H:
                        clipped[y, x] = True
                        continue
                    taps.append((w[dy + r] * w[dx + r], sx, sy))
            if counts is not None:
                same[y, x] = all(counts[sy, sx] == counts[y, x] for _, sx, sy in taps)
            a = [0.0, 0.0, 0.0]
            s = 0.0
            for wgt, sx, sy in taps:
                v = Sl[sy][sx]
                if not same[y, x]:
                    inv = 1.0 / float(counts[sy, sx])
                    v = [v[0] * inv, v[1] * inv, v[2] * inv]
                a[0] = fma(wgt, v[0], a[0])
                a[1] = fma(wgt, v[1], a[1])
                a[2] = fma(wgt, v[2], a[2])
                s = s + wgt
            acc[y, x] = a
            ws[y, x] = s
    return acc, ws, clipped, same


def finish(acc, ws, clipped, flags, spp=None, counts=None, same=None):
    """From accumulate's sums to the image: the renormalisation, the 1 / spp (or 1 / n where `same`), the square root"""
    out = acc.copy()
    if flags & RENORMALISE:
        out[clipped] = out[clipped] / ws[clipped][:, None]
    if counts is None:
        out = out * (1.0 / float(spp))
    else:
        inv = 1.0 / counts.astype(np.float64)
        out[same] = out[same] * inv[same][:, None]
    return np.sqrt(out)


def film(S, order, radius, flags, spp):
    acc, ws, clipped, _ = accumulate(S, order, radius)
    return finish(acc, ws, clipped, flags, spp=spp)


def film_counts(S, counts, order, radius, flags):
    acc, ws, clipped, same = accumulate(S, order, radius, counts)
    return finish(acc, ws, clipped, flags, counts=counts, same=same)


def splat(samples, order, radius):
    """Film_tile for one tile that is the whole image: samples (spp, H, W, 3), pass after pass, each pixel's colour written with
    weight k[dy][dx] to (x + dx, y + dy) of a tile with a border of `radius` pixels by one fma per channel; then stitch_tile: the
    tile's pixels inside the image, added to an image of zeros (v + 0.0).  The pre-sqrt sums (H, W, 3)."""
    spp, H, W, _ = samples.shape
    r = radius
    _, w2 = weights(order, radius)
    tile = [[[0.0, 0.0, 0.0] for _ in range(W + 2 * r)] for _ in range(H + 2 * r)]
    sl = samples.tolist()
    for p in range(spp):
        for y in range(H):
            for x in range(W):
                c = sl[p][y][x]
                for dy in range(-r, r + 1):
                    for dx in range(-r, r + 1):
                        wgt = w2[dy + r][dx + r]
                        px = tile[y + r + dy][x + r + dx]
                        px[0] = fma(wgt, c[0], px[0])
                        px[1] = fma(wgt, c[1], px[1])
                        px[2] = fma(wgt, c[2], px[2])
    img = np.zeros((H, W, 3))
    for ly in range(H + 2 * r):
        for lx in range(W + 2 * r):
            gx, gy = lx - r, ly - r
            if 0 <= gx < W and 0 <= gy < H:
                for ch in range(3):
                    img[gy, gx, ch] = tile[ly][lx][ch] + img[gy, gx, ch]
    return img


def raw_sums(samples):
    """what the render leaves per pixel: the samples added in pass order"""
    S = np.zeros(samples.shape[1:])
    for p in range(samples.shape[0]):
        S = S + samples[p]
    return S


def decades(shape, seed):
    """seeded raw sums over twelve decades with exact zeros"""
    rng = np.random.default_rng(seed)
    S = rng.uniform(1.0, 10.0, shape) * 10.0 ** rng.integers(-6, 6, shape)
    S[rng.random(shape) < 0.1] = 0.0
    return S
