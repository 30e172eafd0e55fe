"""The display rule of include/ptx.h ("display outputs") restated in numpy from the header's text, and the images of edge values the
display tests share.  numpy's binary64 +, *, / are IEEE and unfused, so the restatement computes the rule's own bits; the sRGB codes
are a searchsorted over the table the library hands out (ptx_display_thresholds), the binary32 formats numpy's astype(float32)."""
import numpy as np

FORMATS = ("rgb8", "rgba8", "rgb32f", "rgba32f")
TRANSFERS = ("reference", "linear", "srgb")
TONES = ("none", "reinhard", "aces")
EXPOSURES = (0.0, 2.0 ** -20, 1.0, 2.0 ** 20)
CAP = 2.0 ** 40


def settings():
    """every (format, transfer, tone, exposure) the library accepts at the exposures the tests use"""
    out = []
    for fmt in FORMATS:
        out.append((fmt, "reference", "none", 1.0))
        for transfer in ("linear", "srgb"):
            if transfer == "srgb" and fmt.endswith("32f"):
                continue
            for tone in TONES:
                for e in EXPOSURES:
                    out.append((fmt, transfer, tone, e))
    return out


def value(v, transfer, tone, exposure):
    """Stage A"""
    v = np.asarray(v, dtype=np.float64)
    if transfer == "reference":
        return v.copy()
    with np.errstate(all="ignore"):
        L = (v * v) * np.float64(exposure)
        L = np.where(L > CAP, CAP, L)
        if tone == "reinhard":
            return L / (1.0 + L)
        if tone == "aces":
            return (L * ((2.51 * L) + 0.03)) / ((L * ((2.43 * L) + 0.59)) + 0.14)
        return L


def apply(image, thresholds, fmt="rgb8", transfer="reference", tone="none", exposure=1.0):
    """the display of a float64 array of shape (..., 3): uint8 or float32, shape (..., 3 or 4)"""
    image = np.asarray(image, dtype=np.float64)
    t = value(image, transfer, tone, exposure)
    with np.errstate(all="ignore"):
        if fmt.endswith("32f"):
            body, alpha = t.astype(np.float32), np.float32(1.0)
        elif transfer == "srgb":
            # the number of k with T[k] <= t: the insertion point to the right of equal entries; NaN -> 0
            body = np.where(np.isnan(t), 0, np.searchsorted(thresholds, np.where(np.isnan(t), 0.0, t), side="right")).astype(np.uint8)
            alpha = np.uint8(255)
        else:
            y = t * 255.0
            y = np.where(y > 0.0, y, 0.0)  # !(y > 0): NaN, zeros and negatives
            y = np.where(y > 255.0, 255.0, y)
            body, alpha = y.astype(np.int64).astype(np.uint8), np.uint8(255)  # truncation
    if fmt in ("rgb8", "rgb32f"):
        return body
    out = np.empty(image.shape[:-1] + (4,), dtype=body.dtype)
    out[..., :3] = body
    out[..., 3] = alpha
    return out


def _neighbours(x):
    x = np.atleast_1d(np.asarray(x, dtype=np.float64))
    return np.concatenate([np.nextafter(x, -np.inf), x, np.nextafter(x, np.inf)])


def edge_values(thresholds):
    """the channel values where the rule can go wrong, for v directly (REFERENCE) and, through sqrt, for L = v * v"""
    k = np.arange(256) / 255.0
    f32_tiny = np.float64(np.finfo(np.float32).tiny)  # 2^-126
    f32_sub = np.float64(2.0 ** -149)
    lin = np.concatenate([
        _neighbours(k), _neighbours(thresholds),
        [0.0, -0.0, 5e-324, -5e-324, 2.2250738585072014e-308, 1e-310],
        # values that round into, inside and out of the binary32 subnormal range, ties included
        _neighbours([f32_tiny, f32_sub, 0.5 * f32_sub, 1.5 * f32_sub, 2.5 * f32_sub, f32_tiny - 0.5 * f32_sub, 3.0 * f32_sub,
                     1e-40, 1e-42, 1e-45, 7e-46]),
        -np.array([f32_tiny, f32_sub, 0.5 * f32_sub, 1e-40]),
        _neighbours([CAP, 3.4028234663852886e38, 3.4028235677973366e38, 1.0, 255.0 / 256.0]),
        [1e300, np.inf, -np.inf, np.nan, -1.0, -0.25, -1e300, 0.5, 2.0, 400.0, 6000.0],
    ])
    with np.errstate(all="ignore"):
        roots = np.sqrt(np.abs(lin[np.isfinite(lin)]))  # v whose square lands on or beside each value
        # under each exposure the cap sits at v = sqrt(CAP / e)
        caps = np.concatenate([_neighbours(np.sqrt(CAP / e)) for e in EXPOSURES if e > 0.0])
    return np.concatenate([lin, roots, _neighbours(roots[:64]), caps, -roots[:32]])


def edge_image(thresholds, n_pixels, seed=0):
    """(n_pixels, 3) of edge values: a deterministic draw that covers every value when n_pixels allows, channels mixed"""
    vals = edge_values(thresholds)
    rng = np.random.default_rng(seed)
    flat = vals[rng.integers(0, len(vals), size=n_pixels * 3)]
    m = min(len(vals), n_pixels * 3)
    flat[:m] = vals[rng.permutation(len(vals))[:m]]
    return flat.reshape(n_pixels, 3)


def full_edge_image(thresholds):
    """every edge value at least once: (ceil(n / 3), 3)"""
    vals = edge_values(thresholds)
    n = -(-len(vals) // 3)
    flat = np.resize(vals, n * 3)
    return flat.reshape(n, 3)


def same(a, b):
    """bit for bit, NaN payloads aside (a binary32 NaN is a NaN on both sides)"""
    a, b = np.asarray(a), np.asarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    if a.dtype == np.float32:
        na, nb = np.isnan(a), np.isnan(b)
        return bool(np.array_equal(na, nb) and np.array_equal(np.where(na, 0, a.view(np.uint32)), np.where(nb, 0, b.view(np.uint32))))
    return bool(np.array_equal(a, b))
