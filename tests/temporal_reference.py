"""Temporal accumulation (include/ptx.h, "temporal accumulation: the frame history reprojected across camera poses") restated in numpy,
from the header's text.  numpy's binary64 * + - / sqrt and floor are single IEEE operations, never fused, and the direction d comes
from camera_pose_reference.pose_rays, so every value here is what the rule says bit for bit.

    accumulate(W, H, k, kf, raw, sq, feat, hist_prev, cur, prev, params) -> dict
      raw, sq (H*W, 3), feat (H*W, 8), hist_prev (H*W, 12) or None; cur, prev = (origin, rotation, cam4); params = (cap, normal
      threshold, depth tolerance, min weight)
      keys: hist (H*W, 12), raw_out, err, motion (H*W, 3), count, fx, fy (the reprojected position, NaN where there is none) and
      masks: a dict of per-pixel booleans, one per branch of the rule (MASKS)

    synthetic(W, H, pair, seed) -> the seeded inputs the CPU and GPU tests share, for one of the camera PAIRS
"""
import numpy as np

import camera_pose_reference as CPR

HISTORY_DOUBLES = 12
DEFAULTS = (64.0, 0.9, 0.02, 2.0 ** -10)
MASKS = ("behind", "off_image", "tap_outside", "tap_empty", "tap_kind", "tap_normal", "tap_depth", "tap_taken", "no_history",
         "history", "capped", "miss", "part_hit")


def _cam(c):
    o, R, cam4 = c
    return np.asarray(o, dtype=np.float64).reshape(3), np.asarray(R, dtype=np.float64).reshape(3, 3), tuple(np.float64(v) for v in cam4)


def accumulate(W, H, k, kf, raw, sq, feat, hist_prev, cur, prev, params=DEFAULTS):
    cap, nthr, dtol, minw = (np.float64(v) for v in params)
    n_pix = W * H
    raw, sq, feat = (np.asarray(a, dtype=np.float64).reshape(n_pix, -1) for a in (raw, sq, feat))
    kd, kfd = np.float64(k), np.float64(kf)
    ys, xs = np.divmod(np.arange(n_pix), W)
    xd, yd = xs.astype(np.float64), ys.astype(np.float64)
    Wd, Hd = np.float64(W), np.float64(H)
    with np.errstate(all="ignore"):
        mu, nu = raw / kd, sq / kd
        h = feat[:, 7]
        hf = h / kfd
        n = feat[:, 3:6] / kfd
        hit = h > 0.0
        z = np.where(hit, feat[:, 6] / np.where(hit, h, 1.0), 0.0)
        masks = {m: np.zeros(n_pix, dtype=bool) for m in MASKS}
        masks["miss"] = ~hit
        masks["part_hit"] = hit & (h < kfd)
        fx = np.full(n_pix, np.nan)
        fy = np.full(n_pix, np.nan)
        sw = np.zeros(n_pix)
        a1, a2, aN = np.zeros((n_pix, 3)), np.zeros((n_pix, 3)), np.zeros(n_pix)
        history = np.zeros(n_pix, dtype=bool)
        if hist_prev is not None:
            hp = np.asarray(hist_prev, dtype=np.float64).reshape(n_pix, HISTORY_DOUBLES)
            o, R, cam4 = _cam(cur)
            po, pR, (pllx, plly, pvx, pvy) = _cam(prev)
            cx = (xd + 0.5) * (np.float64(1.0) / Wd)
            cy = 1.0 - (yd + 0.5) * (np.float64(1.0) / Hd)
            _, d = CPR.pose_rays(cam4, o, R, np.stack([cx, cy], axis=1))
            P = np.stack([o[i] + z * d[:, i] for i in range(3)], axis=1)
            v = np.where(hit[:, None], np.stack([P[:, i] - po[i] for i in range(3)], axis=1), d)
            c = np.stack([(pR[0, i] * v[:, 0] + pR[1, i] * v[:, 1]) + pR[2, i] * v[:, 2] for i in range(3)], axis=1)
            front = c[:, 2] < 0.0
            masks["behind"] = ~front
            iz = -c[:, 2]
            qx, qy = c[:, 0] / iz, c[:, 1] / iz
            fx = ((qx - pllx) / pvx) * Wd - 0.5
            fy = (1.0 - (qy - plly) / pvy) * Hd - 0.5
            inside = front & (fx > -1.0) & (fx < Wd) & (fy > -1.0) & (fy < Hd)
            masks["off_image"] = front & ~inside
            fx = np.where(front, fx, np.nan)
            fy = np.where(front, fy, np.nan)
            xf, yf = np.floor(np.where(inside, fx, 0.0)), np.floor(np.where(inside, fy, 0.0))
            x0, y0 = xf.astype(np.int64), yf.astype(np.int64)
            tx, ty = fx - xf, fy - yf
            dist = np.sqrt((v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1]) + v[:, 2] * v[:, 2])
            for j in (0, 1):
                for i in (0, 1):
                    qxi, qyi = x0 + i, y0 + j
                    in_img = (qxi >= 0) & (qxi < W) & (qyi >= 0) & (qyi < H)
                    masks["tap_outside"] |= inside & ~in_img
                    live = inside & in_img
                    rec = hp[np.where(live, qyi * W + qxi, 0)]
                    full = rec[:, 6] > 0.0
                    masks["tap_empty"] |= live & ~full
                    live = live & full
                    kind = np.where(hit, rec[:, 7] > 0.0, rec[:, 7] == 0.0)
                    masks["tap_kind"] |= live & ~kind
                    live = live & kind
                    dot = (n[:, 0] * rec[:, 8] + n[:, 1] * rec[:, 9]) + n[:, 2] * rec[:, 10]
                    normal_ok = ~hit | (dot >= nthr)
                    masks["tap_normal"] |= live & ~normal_ok
                    live = live & normal_ok
                    depth_ok = ~hit | (np.abs(dist - rec[:, 11]) <= dtol * dist)
                    masks["tap_depth"] |= live & ~depth_ok
                    live = live & depth_ok
                    masks["tap_taken"] |= live
                    w = (tx if i else 1.0 - tx) * (ty if j else 1.0 - ty)
                    sw = np.where(live, sw + w, sw)
                    a1 = np.where(live[:, None], a1 + w[:, None] * rec[:, 0:3], a1)
                    a2 = np.where(live[:, None], a2 + w[:, None] * rec[:, 3:6], a2)
                    aN = np.where(live, aN + w * rec[:, 6], aN)
            history = inside & (sw > minw)
        masks["history"] = history
        masks["no_history"] = ~history
        swd = np.where(history, sw, 1.0)
        H1, H2, NH = a1 / swd[:, None], a2 / swd[:, None], aN / swd
        masks["capped"] = history & (NH > cap)
        NH = np.where(NH > cap, cap, NH)
        al = kd / (NH + kd)
        M1 = np.where(history[:, None], H1 * (1.0 - al)[:, None] + mu * al[:, None], mu)
        M2 = np.where(history[:, None], H2 * (1.0 - al)[:, None] + nu * al[:, None], nu)
        N = np.where(history, NH + kd, kd)
        hist = np.concatenate([M1, M2, N[:, None], hf[:, None], n, z[:, None]], axis=1)
        var = M2 - M1 * M1
        var = np.where(var > 0.0, var, 0.0)
        err = np.sqrt(var / (N - 1.0)[:, None])
        motion = np.where(history[:, None], np.stack([fx - xd, fy - yd, sw], axis=1), 0.0)
    return {"hist": hist, "raw_out": M1 * kd, "err": err, "motion": motion, "count": int(history.sum()), "fx": fx, "fy": fy,
            "masks": masks, "mu": mu, "nu": nu}


# ------------------------------------------------------------------------------------------------ the synthetic inputs
def rotation(axis, angle):
    a = np.asarray(axis, dtype=np.float64)
    a = a / np.linalg.norm(a)
    K = np.array([[0.0, -a[2], a[1]], [a[2], 0.0, -a[0]], [-a[1], a[0], 0.0]])
    return np.eye(3) + np.sin(angle) * K + (1.0 - np.cos(angle)) * (K @ K)


VIEW = (-1.0, -0.5, 2.0, 1.0)
PAIRS = ("identical", "moved", "views", "turned_away", "null")
SIZES = ((1, 1), (1, 40), (40, 1), (33, 31), (70, 45))
K, KF = 4, 3


def cameras(pair):
    """(current, previous) cameras of a pair; previous is None for "null" """
    cur = (np.array([0.2, -0.1, 0.3]), rotation((0.1, 1.0, 0.2), 0.05), VIEW)
    if pair in ("identical", "null"):
        return cur, (None if pair == "null" else cur)
    if pair == "moved":
        return cur, (np.array([0.05, 0.02, 0.4]), rotation((0.3, 1.0, -0.1), 0.02), VIEW)
    if pair == "views":
        return cur, (cur[0], cur[1], (-0.8, -0.2, 1.3, 0.9))
    if pair == "turned_away":
        return cur, (cur[0], rotation((0.0, 1.0, 0.0), np.pi) @ cur[1], VIEW)
    raise KeyError(pair)


def _plane_features(W, H, cam, kf):
    """the analytic first hits of a wall z = -4 facing +z, seen from `cam`: (hit distance t, valid) per pixel"""
    o, R, cam4 = _cam(cam)
    ys, xs = np.divmod(np.arange(W * H), W)
    cxcy = np.stack([(xs + 0.5) / W, 1.0 - (ys + 0.5) / H], axis=1)
    _, d = CPR.pose_rays(cam4, o, R, cxcy)
    with np.errstate(all="ignore"):
        t = (-4.0 - o[2]) / d[:, 2]
    return t, np.isfinite(t) & (t > 0.0)


def synthetic(W, H, pair, seed=0):
    """Seeded sums, features and a previous history for a W x H frame under one of PAIRS.  The world is a wall at z = -4 with a sky
    band across the frame's middle; a share of the pixels hit in only some feature passes; the previous history is the wall seen from
    the previous camera, with records knocked out in every way the rule rejects one: N = 0, a hit where the frame has sky and the
    other way round, a turned normal, a wrong depth, and N above the cap."""
    rng = np.random.default_rng([seed, W, H, PAIRS.index(pair)])
    n_pix = W * H
    cur, prev = cameras(pair)
    ys, xs = np.divmod(np.arange(n_pix), W)
    raw = rng.uniform(0.0, 4.0, (n_pix, 3)) * K
    sq = raw * raw / K + rng.uniform(0.0, 2.0, (n_pix, 3)) * K  # S2 >= S1^2 / k
    t, ok = _plane_features(W, H, cur, KF)
    sky = ~ok | ((xs + ys) % 7 == 3)
    h = np.where(sky, 0.0, np.where(rng.random(n_pix) < 0.25, float(KF - 1), float(KF)))
    feat = np.zeros((n_pix, 8))
    feat[:, 0:3] = rng.uniform(0.0, 1.0, (n_pix, 3)) * KF
    feat[:, 5] = h  # the wall's normal (0, 0, 1), summed over the passes that hit
    feat[:, 6] = np.where(sky, 0.0, t) * h
    feat[:, 7] = h
    hist = None
    if prev is not None or pair == "null":
        pt, pok = _plane_features(W, H, prev if prev is not None else cur, KF)
        hist = np.zeros((n_pix, HISTORY_DOUBLES))
        hist[:, 0:3] = rng.uniform(0.0, 4.0, (n_pix, 3))
        hist[:, 3:6] = hist[:, 0:3] ** 2 + rng.uniform(0.0, 2.0, (n_pix, 3))
        hist[:, 6] = rng.choice([4.0, 12.0, 40.0, 64.0, 90.5, 200.0], n_pix)
        psky = ~pok | ((xs + ys) % 7 == 3)
        hist[:, 7] = np.where(psky, 0.0, 1.0)
        hist[:, 10] = np.where(psky, 0.0, 1.0)
        hist[:, 11] = np.where(psky, 0.0, pt)
        u = rng.random(n_pix)
        hist[:, 6] = np.where(u < 0.12, 0.0, hist[:, 6])                                   # no record
        flip = (u >= 0.12) & (u < 0.24)                                                    # hit <-> sky
        hist[:, 7] = np.where(flip, np.where(psky, 1.0, 0.0), hist[:, 7])
        turn = (u >= 0.24) & (u < 0.36) & ~psky                                            # a turned normal
        hist[:, 8] = np.where(turn, 0.8, hist[:, 8])
        hist[:, 10] = np.where(turn, 0.6, hist[:, 10])
        far = (u >= 0.36) & (u < 0.48) & ~psky                                             # a wrong depth
        hist[:, 11] = np.where(far, hist[:, 11] * 1.25, hist[:, 11])
    return {"W": W, "H": H, "k": K, "kf": KF, "raw": raw, "sq": sq, "feat": feat, "hist": None if pair == "null" else hist,
            "cur": cur, "prev": prev}
