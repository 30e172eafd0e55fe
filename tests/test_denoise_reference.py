"""The a-trous rule (tests/denoise_reference.py, the numpy restatement of include/ptx.h's ptx_denoise_device) on the CPU: its
identities, and its quality on the oracle's per-sample radiance with first-hit features restated from the oracle's camera rays and
closest hits."""
import numpy as np
import pytest

import denoise_reference as R

EPS = 2.0 ** -53


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _uniform_features(H, W, kf, albedo=(0.5, 0.25, 0.75), normal=(0.0, 0.6, 0.8), depth=3.0):
    feat = np.zeros((H, W, 8))
    feat[..., 0:3] = np.array(albedo) * kf
    feat[..., 3:6] = np.array(normal) * kf
    feat[..., 6] = depth * kf
    feat[..., 7] = kf
    return feat


def test_levels_zero_is_the_identity():
    rng = np.random.default_rng(1)
    raw = rng.uniform(0.0, 9.0, (7, 5, 3))
    out = R.denoise(raw, rng.uniform(0.1, 1.0, (7, 5, 3)), _uniform_features(7, 5, 4), 8, 4, levels=0)
    assert np.array_equal(bits(out), bits(raw))


@pytest.mark.parametrize("levels", [1, 3, 5])
@pytest.mark.parametrize("flags", [0, R.DEMODULATE])
def test_a_constant_image_stays_constant(levels, flags):
    """uniform features, one colour, any positive variance: every level is sum(w c) / sum(w) of equal c -- 25 products and 48
    additions of non-negative terms plus one division per level, each within 2^-53 relative"""
    rng = np.random.default_rng(2)
    H, W, k = 37, 41, 8
    colour = np.array([0.7, 1.9, 0.05])
    raw = np.broadcast_to(colour * k, (H, W, 3)).copy()
    err = rng.uniform(1e-3, 2.0, (H, W, 3))
    out = R.denoise(raw, err, _uniform_features(H, W, 4), k, 4, levels=levels, flags=flags)
    rel = np.abs(out - raw) / raw
    assert rel.max() <= 60 * levels * EPS, rel.max()


def test_orthogonal_half_planes_do_not_bleed():
    """w_n is exactly 0 across the edge: each half is a constant image of its own"""
    rng = np.random.default_rng(3)
    H, W, k, kf, L = 40, 48, 6, 3, 5
    c1, c2 = np.array([2.0, 0.5, 0.25]), np.array([0.1, 3.0, 1.5])
    raw = np.zeros((H, W, 3))
    raw[:, : W // 2] = c1 * k
    raw[:, W // 2:] = c2 * k
    feat = _uniform_features(H, W, kf, normal=(1.0, 0.0, 0.0))
    feat[:, W // 2:, 3:6] = np.array([0.0, 0.0, 1.0]) * kf
    err = rng.uniform(0.05, 3.0, (H, W, 3))
    out = R.denoise(raw, err, feat, k, kf, levels=L)
    rel = np.abs(out - raw) / raw
    assert rel.max() <= 60 * L * EPS, rel.max()


def test_a_count_map_scales_each_pixel_by_its_own_count():
    rng = np.random.default_rng(4)
    H, W = 9, 11
    counts = rng.integers(2, 10, (H, W)).astype(np.int32)
    mean = rng.uniform(0.1, 2.0, (H, W, 3))
    feat = _uniform_features(H, W, 2)
    err = rng.uniform(0.01, 0.5, (H, W, 3))
    a = R.denoise(mean * counts[..., None], err, feat, counts, 2, levels=2)
    b = R.denoise(mean * 4.0, err, feat, 4, 2, levels=2)
    assert np.allclose(a / counts[..., None], b / 4.0, rtol=1e-12)


# ---------------------------------------------------------------- quality on the oracle's samples
def first_hit_features(oracle, d, W, H, N, depth, k):
    """Feature sums (H, W, 8) over passes [0, k) of the N-pass frame: a plain numpy restatement of the first hit on the oracle's
    camera rays (orc_lds_get, orc_camera_ray) and closest hits (orc_intersect_rays)."""
    L = oracle.lib()
    A = d.arrays()
    dim = 2 + 2 * depth
    cam = np.ascontiguousarray(A["camera"])
    ys, xs, ps = (a.ravel() for a in np.meshgrid(np.arange(H), np.arange(W), np.arange(k), indexing="ij"))
    n = len(xs)
    D = np.zeros((n, 3))
    ray = np.zeros(6)
    for i in range(n):
        off = int(ys[i]) * W + int(xs[i]) + int(ps[i]) * N
        cx = (float(xs[i]) + L.orc_lds_get(dim, off, 0)) * (1.0 / W)
        cy = 1.0 - ((float(ys[i]) + L.orc_lds_get(dim, off, 1)) * (1.0 / H))
        L.orc_camera_ray(oracle._dp(cam), cx, cy, oracle._dp(ray))
        D[i] = ray[3:]
    O = np.zeros((n, 3))
    sc = oracle.Scene(d.ptr, d)
    t, prim, _ = sc.intersect_rays(O, D)
    sc.close()
    nt, ns = len(A["tri_material"]), len(A["sphere_material"])
    hit = prim >= 0
    normal = np.zeros((n, 3))
    tu, tv = np.zeros(n), np.zeros(n)
    mat = np.zeros(n, dtype=np.int64)
    point = D * t[:, None]
    sph = hit & (prim >= nt) & (prim < nt + ns)
    if sph.any():
        s = prim[sph] - nt
        c = np.stack([A["sphere_x"][s], A["sphere_y"][s], A["sphere_z"][s]], axis=1)
        nn = point[sph] - c
        nn /= np.linalg.norm(nn, axis=1)[:, None]
        nn = np.where((np.einsum("ij,ij->i", D[sph], nn) < 0.0)[:, None], nn, -nn)
        normal[sph] = nn
        tu[sph] = (np.pi + np.arctan2(-nn[:, 2], nn[:, 0])) / (2.0 * np.pi)
        tv[sph] = np.arccos(np.clip(-nn[:, 1], -1.0, 1.0)) / np.pi
        mat[sph] = A["sphere_material"][s]
    tri = hit & ~sph
    if tri.any():
        p = prim[tri]
        fl = p >= nt + ns
        V = np.stack([A["vertex_x"], A["vertex_y"], A["vertex_z"]], axis=1) if nt else np.zeros((1, 3))
        idx = A["tri_indices"].reshape(-1, 3) if nt else np.zeros((1, 3), dtype=np.int64)
        tv3 = V[idx[np.clip(p, 0, max(nt - 1, 0))]]  # (m, 3, 3)
        if fl.any():
            tv3[fl] = A["floor_vertices"].reshape(-1, 3, 3)[p[fl] - nt - ns]
        a, b, c = tv3[:, 0], tv3[:, 1], tv3[:, 2]
        gn = np.cross(b - a, c - a)
        gn /= np.linalg.norm(gn, axis=1)[:, None]
        gn = np.where((np.einsum("ij,ij->i", D[tri], gn) < 0.0)[:, None], gn, -gn)
        normal[tri] = gn
        # barycentrics of the hit point, for the texture coordinates
        e1, e2, q = b - a, c - a, point[tri] - a
        d11, d12, d22 = (e1 * e1).sum(1), (e1 * e2).sum(1), (e2 * e2).sum(1)
        q1, q2 = (q * e1).sum(1), (q * e2).sum(1)
        det = d11 * d22 - d12 * d12
        u, v = (d22 * q1 - d12 * q2) / det, (d11 * q2 - d12 * q1) / det
        uv = np.zeros((len(p), 6))
        if nt:
            uv[~fl] = A["tri_uv"].reshape(-1, 6)[p[~fl]]
        if fl.any():
            uv[fl] = A["floor_uv"].reshape(-1, 6)[p[fl] - nt - ns]
        w = 1.0 - u - v
        tu[tri] = uv[:, 0] * w + uv[:, 2] * u + uv[:, 4] * v
        tv[tri] = uv[:, 1] * w + uv[:, 3] * u + uv[:, 5] * v
        m = np.zeros(len(p), dtype=np.int64)
        if nt:
            m[~fl] = A["tri_material"][p[~fl]]
        if fl.any():
            m[fl] = A["floor_material"][p[fl] - nt - ns]
        mat[tri] = m
    M, T = A["materials"], A["textures"]
    kind = M[mat, 0].astype(int)
    tex = T[np.clip(M[mat, 1].astype(int), 0, len(T) - 1)]
    px = np.trunc(tu * (tex[:, 1] - 1)).astype(np.int64) & 1
    py = np.trunc(tv * (tex[:, 2] - 1)).astype(np.int64) & 1
    even = (tex[:, 0] == 0) | (px == py)
    albedo = np.where(even[:, None], tex[:, 3:6], tex[:, 6:9])
    albedo = np.where((kind == 2)[:, None], 1.0, albedo)
    bg = A["background"]
    if bg[0] == 0:
        sky = np.zeros((n, 3))
    else:
        tt = 0.5 * (D[:, 1] / np.linalg.norm(D, axis=1) + 1.0)
        sky = (1.0 - tt)[:, None] * bg[1:4] + tt[:, None] * bg[4:7]
    rec = np.zeros((n, 8))
    rec[:, 0:3] = np.where(hit[:, None], albedo, sky)
    rec[:, 3:6] = np.where(hit[:, None], normal, 0.0)
    rec[:, 6] = np.where(hit, t, 0.0)
    rec[:, 7] = hit
    rec = rec.reshape(H, W, k, 8)
    feat = np.zeros((H, W, 8))
    for j in range(k):
        feat = feat + rec[:, :, j]
    return feat


def sample_sums(oracle, d, W, H, N, depth):
    ys, xs, ps = np.meshgrid(np.arange(H), np.arange(W), np.arange(N), indexing="ij")
    sc = oracle.Scene(d.ptr, d)
    rgb, _ = sc.trace_samples(W, H, N, depth, xs.ravel(), ys.ravel(), ps.ravel())
    sc.close()
    per = rgb.reshape(H, W, N, 3)
    s1, s2 = np.zeros((H, W, 3)), np.zeros((H, W, 3))
    for p in range(N):
        c = per[:, :, p]
        s1 = s1 + c
        s2 = s2 + c * c
    return s1, s2


def rmse(a, b):
    return float(np.sqrt(np.mean((a - b) ** 2)))


def quality_ratio(oracle, d, W, H, N, depth, reference_spp=512, **settings):
    """(noisy linear RMSE, denoised linear RMSE) against the oracle's reference_spp raw mean, at the given settings"""
    s1, s2 = sample_sums(oracle, d, W, H, N, depth)
    kw = dict(R.DEFAULTS)
    kw.update(settings)
    F = kw.pop("feature_passes")
    kf = min(F, N) if F > 0 else N
    feat = first_hit_features(oracle, d, W, H, N, depth, kf)
    out = R.denoise(s1, R.standard_error(s1, s2, N), feat, N, kf, **kw)
    sc = oracle.Scene(d.ptr, d)
    ref = sc.render(W, H, reference_spp, depth, threads=4, want_raw=True)["raw"] / reference_spp
    sc.close()
    return rmse(s1 / N, ref), rmse(out / N, ref)


@pytest.mark.slow
def test_cornell_at_8_passes_halves_the_error(oracle):
    """cornell 64x64, N = 8, depth 8, the defaults: linear-mean RMSE < 0.5 x the noisy one (the prototype measured 0.33)"""
    noisy, den = quality_ratio(oracle, oracle.desc_cornell(64, 64), 64, 64, 8, 8)
    print(f"\ncornell 64x64 spp 8: noisy {noisy:.4f} denoised {den:.4f} ratio {den / noisy:.3f}")
    assert den < 0.5 * noisy, (noisy, den)


@pytest.mark.slow
def test_shirley_at_4_passes_is_not_made_worse(oracle):
    """Shirley 96x48, N = 4, depth 8: spheres about a pixel large, < 1 x (the prototype measured 0.96)"""
    noisy, den = quality_ratio(oracle, oracle.desc_shirley(96, 48), 96, 48, 4, 8)
    print(f"\nshirley 96x48 spp 4: noisy {noisy:.4f} denoised {den:.4f} ratio {den / noisy:.3f}")
    assert den < 1.0 * noisy, (noisy, den)
