"""The temporal rule (include/ptx.h, ptx_temporal_accumulate_device) on the CPU: properties of its numpy restatement
(tests/temporal_reference.py), the reach of the synthetic inputs the GPU test compares bit for bit, and what accumulation buys on
real samples -- the restatement's per-sample radiance and first hits (tests/camera_pose_support.Restatement) over an orbit."""
import numpy as np
import pytest

import camera_pose_reference as CPR
import temporal_reference as T


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _run(s, hist="own", cur=None, prev=None, params=T.DEFAULTS):
    return T.accumulate(s["W"], s["H"], s["k"], s["kf"], s["raw"], s["sq"], s["feat"], s["hist"] if isinstance(hist, str) else hist,
                        cur if cur is not None else s["cur"], prev if prev is not None else s["prev"], params)


SIZES = [sz for sz in T.SIZES if sz != (1, 1)]


# ------------------------------------------------------------------------------------------------ (a)
@pytest.mark.parametrize("W,H", T.SIZES)
def test_the_same_camera_reprojects_every_pixel_onto_itself(W, H):
    s = T.synthetic(W, H, "identical")
    first = _run(s, hist=None)
    assert first["count"] == 0
    again = _run(s, hist=first["hist"], prev=s["cur"])
    ys, xs = np.divmod(np.arange(W * H), W)
    assert np.abs(again["fx"] - xs).max() <= 1e-9 and np.abs(again["fy"] - ys).max() <= 1e-9
    full = s["feat"][:, 7] == s["kf"]
    assert full.any() or (W, H) == (1, 1)
    assert again["masks"]["history"][full].all()
    sky = s["feat"][:, 7] == 0.0
    assert again["masks"]["history"][sky].all()  # a miss finds the miss it wrote
    m = again["motion"][again["masks"]["history"]]
    assert np.abs(m[:, :2]).max() <= 1e-9 and np.abs(m[:, 2] - 1.0).max() <= 1e-9


# ------------------------------------------------------------------------------------------------ (b)
@pytest.mark.parametrize("W,H", SIZES)
def test_a_turn_about_the_cameras_own_origin_moves_pixels_whatever_their_depth(W, H):
    s = T.synthetic(W, H, "identical")
    rng = np.random.default_rng(5)
    feat = s["feat"].copy()
    hit = feat[:, 7] > 0
    feat[:, 6] = np.where(hit, rng.uniform(0.1, 1e4, W * H) * feat[:, 7], 0.0)  # any depth
    o, R1, view = s["cur"]
    R0 = T.rotation((0.2, 1.0, 0.1), 0.03) @ R1
    got = T.accumulate(W, H, s["k"], s["kf"], s["raw"], s["sq"], feat, s["hist"], (o, R1, view), (o, R0, view))
    ys, xs = np.divmod(np.arange(W * H), W)
    _, d = CPR.pose_rays(view, o, R1, np.stack([(xs + 0.5) / W, 1.0 - (ys + 0.5) / H], axis=1))
    c = d @ R0  # rows: R0^T d
    assert (c[:, 2] < 0).all()
    fx = ((c[:, 0] / -c[:, 2] - view[0]) / view[2]) * W - 0.5
    fy = (1.0 - (c[:, 1] / -c[:, 2] - view[1]) / view[3]) * H - 0.5
    assert hit.any()
    dx, dy = np.abs(got["fx"] - fx), np.abs(got["fy"] - fy)
    print(f"\n{W}x{H}: largest |fx - expected| {dx.max():.3g}, |fy - expected| {dy.max():.3g}")
    assert dx[hit].max() <= 1e-9 and dy[hit].max() <= 1e-9
    assert dx[~hit].max(initial=0.0) <= 1e-9 and dy[~hit].max(initial=0.0) <= 1e-9 and np.abs(fx - xs).max() > 1e-3


# ------------------------------------------------------------------------------------------------ (c)
@pytest.mark.parametrize("W,H", T.SIZES)
def test_no_history_returns_the_frame_bit_for_bit(W, H):
    s = T.synthetic(W, H, "moved")
    for hist in (None, np.zeros((W * H, T.HISTORY_DOUBLES))):
        r = _run(s, hist=hist)
        assert r["count"] == 0 and not r["motion"].any()
        assert np.array_equal(bits(r["hist"][:, 0:3]), bits(r["mu"])) and np.array_equal(bits(r["hist"][:, 3:6]), bits(r["nu"]))
        assert (r["hist"][:, 6] == s["k"]).all()
        assert np.array_equal(bits(r["raw_out"]), bits(r["mu"] * np.float64(s["k"])))
    capless = _run(s, params=(0.0,) + T.DEFAULTS[1:])
    assert np.array_equal(bits(capless["hist"][:, 0:3]), bits(capless["mu"])) and (capless["hist"][:, 6] == s["k"]).all()
    if (W, H) != (1, 1):
        assert capless["count"] > 0 and capless["count"] == _run(s)["count"]


# ------------------------------------------------------------------------------------------------ (d)
@pytest.mark.parametrize("W,H", SIZES)
def test_the_synthetic_inputs_reach_every_branch(W, H):
    reached = {m: False for m in T.MASKS}
    for pair in T.PAIRS:
        r = _run(T.synthetic(W, H, pair))
        for m in T.MASKS:
            reached[m] |= bool(r["masks"][m].any())
        if pair == "turned_away":
            assert r["masks"]["behind"].all() and r["count"] == 0
        if pair == "null":
            assert r["count"] == 0
        if pair in ("identical", "moved"):
            assert 0 < r["count"] < W * H, pair
    assert all(reached.values()), [m for m, v in reached.items() if not v]


# ------------------------------------------------------------------------------------------------ (e)
def _orbit(F, deg):
    """the camera `deg` degrees along an orbit about the point the scene's own camera looks at from distance F"""
    R = T.rotation((0.0, 1.0, 0.0), np.radians(deg))
    pivot = np.array([0.0, 0.0, -F])
    return pivot + R @ np.array([0.0, 0.0, F]), R


def _frame(c, S, pose, W, H, N, depth, first, count):
    xs, ys, ps = S.all_samples(W, H, count)
    ps = S.i32(ps + first)
    rgb, _ = c["ref"].trace_samples(pose, W, H, N, depth, xs, ys, ps, c["images"], c["env"], 0, c["sampling"])
    feat = c["ref"].first_hits(pose, W, H, N, depth, xs, ys, ps, c["images"], c["env"])
    raw, sq, fs = np.zeros((W * H, 3)), np.zeros((W * H, 3)), np.zeros((W * H, 8))
    rgb, feat = rgb.reshape(W * H, count, 3), feat.reshape(W * H, count, 8)
    for p in range(count):  # pass order, as the device sums
        raw = raw + rgb[:, p]
        sq = sq + rgb[:, p] * rgb[:, p]
        fs = fs + feat[:, p]
    return raw, sq, fs


QUALITY = {"shirley": (96, 48, 0.8), "cornell": (64, 64, 0.6)}


@pytest.mark.parametrize("name", list(QUALITY))
def test_accumulation_over_an_orbit_beats_the_single_frame(oracle, name):
    """8 frames of 4 passes of N = 64 on a 1-degree-per-frame orbit against the restatement's 256-spp frame at the last pose.
    The bars (0.8 and 0.6) are the prototype's ratios, 0.66 and 0.39, plus room for the rule's final details; the ideal for 8 equal
    frames is 0.354.  Measured with the rule as it stands, at depth 8 (linear RMSE of the last frame alone, accumulated, their
    ratio, the share of pixels with history over frames 1 .. 7):
      shirley 96 x 48   0.0818   0.0543   0.663   0.78 .. 0.79
      cornell 64 x 64   2.4835   0.9487   0.382   0.90 .. 0.92"""
    import camera_pose_support as S
    W, H, bar = QUALITY[name]
    N, K, frames, depth = 64, 4, 8, 8
    c = S.case(name, oracle, W, H)
    view = S.cam4_of(c["desc"])
    F = c["lens"][1]
    hist = cam = None
    shares = []
    for f in range(frames):
        o, R = _orbit(F, float(f))
        raw, sq, fs = _frame(c, S, S.Pose(o, R), W, H, N, depth, f * K, K)
        r = T.accumulate(W, H, K, K, raw, sq, fs, hist, (o, R, view), cam)
        if f:
            shares.append(r["count"] / (W * H))
        else:
            assert r["count"] == 0
        hist, cam = r["hist"], (o, R, view)
    xs, ys, ps = S.all_samples(W, H, 256)
    want, _ = c["ref"].trace_samples(S.Pose(o, R), W, H, 256, depth, xs, ys, ps, c["images"], c["env"], 0, c["sampling"])
    want = want.reshape(W * H, 256, 3).mean(axis=1)
    alone = float(np.sqrt(np.mean((r["mu"] - want) ** 2)))
    accumulated = float(np.sqrt(np.mean((r["hist"][:, 0:3] - want) ** 2)))
    print(f"\n{name} {W}x{H}: linear RMSE last frame alone {alone:.4f}, accumulated {accumulated:.4f}, ratio {accumulated / alone:.3f}, "
          f"history share {min(shares):.2f}..{max(shares):.2f}")
    assert min(shares) >= 0.5, shares
    assert accumulated / alone <= bar, (alone, accumulated)
    # a 180-degree jump along the orbit: the camera looks at the scene from its far side, and every pixel loses its history --
    # behind the old camera, off its image, or refused by the normal or the depth of what the old frame saw there
    o2, R2 = _orbit(F, float(frames - 1) + 180.0)
    raw, sq, fs = _frame(c, S, S.Pose(o2, R2), W, H, N, depth, frames * K, K)
    j = T.accumulate(W, H, K, K, raw, sq, fs, hist, (o2, R2, view), cam)
    print(f"{name} after the 180-degree jump: history {j['count']} pixels; "
          + ", ".join(f"{m} {int(j['masks'][m].sum())}" for m in T.MASKS))
    assert j["count"] == 0 and not j["masks"]["history"].any() and not j["motion"].any()
    assert np.array_equal(bits(j["raw_out"]), bits(j["mu"] * np.float64(K)))
    assert np.array_equal(bits(j["hist"][:, 0:3]), bits(j["mu"])) and np.array_equal(bits(j["hist"][:, 3:6]), bits(j["nu"]))
    assert (j["hist"][:, 6] == K).all()
