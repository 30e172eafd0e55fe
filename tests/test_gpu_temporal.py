"""Temporal accumulation on the GPU (include/ptx.h, ptx_temporal_accumulate_device / ptx_render_temporal).

* the device function equals the numpy restatement of its rule (tests/temporal_reference.py) bit for bit -- history, sums, error,
  motion and the history count -- on the seeded synthetic inputs whose reach tests/test_temporal_reference.py asserts, at sizes from
  one pixel to ragged many-tile ones and under every camera pair; two runs give the same bits;
* ptx_render_temporal equals the chain of device calls it is documented to be, frame for frame and bit for bit, over posed frames on
  two scenes, without a spatial filter and with the default one;
* what drops the history (a reset, another size) and what does not; a lens is refused; a pose-off scene is the identity pose's
  camera; a plain render on the same handle is untouched.
"""
import ctypes as C

import numpy as np
import pytest

import temporal_reference as T

pytestmark = pytest.mark.gpu
PTX_ERR_ARG, PTX_ERR_STATE = -1, -3


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
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to("cuda:0")


def _zeros(torch, n, c):
    return torch.zeros((n, c), dtype=torch.float64, device="cuda:0")


def _camera(abi, cam):
    return None if cam is None else abi.temporal_camera(*cam)


def _device_run(P, torch, s, params=None, motion=True):
    from path_tracer_ocaml_amd import abi
    n = s["W"] * s["H"]
    d_raw, d_sq, d_feat = _dev(torch, s["raw"]), _dev(torch, s["sq"]), _dev(torch, s["feat"])
    d_prev = None if s["hist"] is None else _dev(torch, s["hist"])
    # outputs start as NaN: a pixel the kernel skipped would show
    d_hist, d_out, d_err, d_mot = (torch.full((n, c), float("nan"), dtype=torch.float64, device="cuda:0") for c in (12, 3, 3, 3))
    took = P.temporal_accumulate_device(0, s["W"], s["H"], params, s["k"], s["kf"], _camera(abi, s["cur"]), _camera(abi, s["prev"]),
                                        d_raw.data_ptr(), d_sq.data_ptr(), d_feat.data_ptr(), None if d_prev is None else d_prev.data_ptr(),
                                        d_hist.data_ptr(), d_out.data_ptr(), d_err.data_ptr(), d_mot.data_ptr() if motion else None)
    return {"hist": d_hist.cpu().numpy(), "raw_out": d_out.cpu().numpy(), "err": d_err.cpu().numpy(), "motion": d_mot.cpu().numpy(),
            "count": took}


def _want(s, params=T.DEFAULTS):
    return T.accumulate(s["W"], s["H"], s["k"], s["kf"], s["raw"], s["sq"], s["feat"], s["hist"], s["cur"], s["prev"], params)


# ------------------------------------------------------------------------------------------------ the device function
@pytest.mark.parametrize("pair", T.PAIRS)
@pytest.mark.parametrize("W,H", T.SIZES)
def test_the_device_function_equals_the_restatement(P, torch, W, H, pair):
    s = T.synthetic(W, H, pair)
    got, want = _device_run(P, torch, s), _want(s)
    for key in ("hist", "raw_out", "err", "motion"):
        nbad = int((bits(got[key]) != bits(want[key])).any(axis=1).sum())
        assert nbad == 0, f"{key}: {nbad} of {W * H} pixels differ ({W} x {H}, {pair})"
    assert got["count"] == want["count"]
    assert np.isfinite(got["err"]).all()


def test_other_settings_equal_the_restatement(P, torch):
    """a cap below every record, a cap of 0, a threshold, a tolerance and a weight everything passes, and ones hardly anything does"""
    s = T.synthetic(70, 45, "moved")
    counts = []
    for params in ((8.0, 0.9, 0.02, 2.0 ** -10), (0.0, 0.9, 0.02, 2.0 ** -10), (1e9, -1.0, 1e3, 0.0), (64.0, 1.0, 0.0, 0.5)):
        got = _device_run(P, torch, s, dict(zip(("max_history_passes", "normal_threshold", "depth_tolerance", "min_weight"), params)))
        want = _want(s, params)
        for key in ("hist", "raw_out", "err", "motion"):
            assert np.array_equal(bits(got[key]), bits(want[key])), (key, params)
        assert got["count"] == want["count"]
        counts.append(got["count"])
    assert counts[0] == counts[1] and counts[2] > counts[0] > counts[3]


def test_two_runs_give_the_same_bits_with_and_without_motion(P, torch):
    s = T.synthetic(70, 45, "moved")
    a, b, c = _device_run(P, torch, s), _device_run(P, torch, s), _device_run(P, torch, s, motion=False)
    for key in ("hist", "raw_out", "err"):
        assert np.array_equal(bits(a[key]), bits(b[key])) and np.array_equal(bits(a[key]), bits(c[key])), key
    assert np.array_equal(bits(a["motion"]), bits(b["motion"])) and a["count"] == b["count"] == c["count"] > 0
    assert np.isnan(c["motion"]).all()  # not asked for: not written


def test_the_device_function_checks_its_arguments(P, torch):
    from path_tracer_ocaml_amd import abi
    W, H = 8, 4
    n = W * H
    z3, z3b, z8, h0, h1, o3, e3 = (_zeros(torch, n, c) for c in (3, 3, 8, 12, 12, 3, 3))
    t, cam = P.temporal_defaults(), abi.temporal_camera(np.zeros(3), np.eye(3), T.VIEW)
    L = P.lib()

    def call(k=4, kf=4, prev=h0, out=h1, raw_out=o3, prev_cam=cam):
        vp = lambda a: None if a is None else C.c_void_p(a.data_ptr())  # noqa: E731
        return L.ptx_temporal_accumulate_device(0, W, H, C.byref(t), k, kf, C.byref(cam), None if prev_cam is None else C.byref(prev_cam), vp(z3),
                                                vp(z3b), vp(z8), vp(prev), vp(out), vp(raw_out), vp(e3), None, None, None)
    assert call() == 0
    assert call(prev=None, prev_cam=None) == 0
    assert call(k=1) == PTX_ERR_ARG and call(kf=0) == PTX_ERR_ARG
    assert call(out=h0) == PTX_ERR_ARG and "must not alias" in P.last_error()
    assert call(raw_out=z3) == PTX_ERR_ARG and "must not alias" in P.last_error()
    assert call(prev_cam=None) == PTX_ERR_ARG and "prev_camera" in P.last_error()
    assert call(out=None) == PTX_ERR_ARG


# ------------------------------------------------------------------------------------------------ one frame of a sequence
W, H, N, K, DEPTH, FRAMES = 64, 48, 16, 4, 4, 4


def _poses(F):
    """a short orbit about the point the scene's own camera looks at, 2 degrees a frame, with a small climb"""
    out = []
    for f in range(FRAMES):
        R = T.rotation((0.1, 1.0, 0.0), np.radians(2.0 * f))
        pivot = np.array([0.0, 0.0, -F])
        out.append((pivot + R @ np.array([0.0, 0.0, F]) + np.array([0.0, 0.01 * f * F, 0.0]), R))
    return out


@pytest.fixture(scope="module")
def cases(oracle):
    import camera_pose_support as S
    return {name: S.case(name, oracle, W, H) for name in ("shirley", "cornell")}


def _scene(P, c):
    import camera_pose_support as S
    return S.gpu_scene(P, c, None)


def _by_hand(P, torch, g, view, frames, denoise, width=W, height=H):
    """frames: (origin, rotation) or None for the pose off.  The chain the header documents, with this test's own buffers."""
    from path_tracer_ocaml_amd import abi
    n = width * height
    params = P.render_params(width, height, N, DEPTH)
    hist = [_zeros(torch, n, 12), _zeros(torch, n, 12)]
    prev_cam, out = None, []
    for f, pose in enumerate(frames):
        if pose is None:
            g.set_camera_pose()
            cam = abi.temporal_camera(np.zeros(3), np.eye(3), view)
        else:
            g.set_camera_pose(*pose)
            cam = abi.temporal_camera(pose[0], pose[1], view)
        raw, sq, feat = _zeros(torch, n, 3), _zeros(torch, n, 3), _zeros(torch, n, 8)
        acc, err, mot, den, rgb = (_zeros(torch, n, 3) for _ in range(5))
        first = (f * K) % N
        g.render_passes_device(params, first, K, raw.data_ptr(), sq.data_ptr())
        g.render_features_device(params, first, K, feat.data_ptr())
        took = P.temporal_accumulate_device(0, width, height, None, K, K, cam, prev_cam, raw.data_ptr(), sq.data_ptr(), feat.data_ptr(),
                                            hist[(f + 1) % 2].data_ptr() if prev_cam is not None else None, hist[f % 2].data_ptr(),
                                            acc.data_ptr(), err.data_ptr(), mot.data_ptr())
        filmed = acc
        if denoise:
            P.denoise_device(0, width, height, None, K, K, acc.data_ptr(), err.data_ptr(), feat.data_ptr(), den.data_ptr())
            filmed = den
        P.film_resolve_device(0, width, height, K, filmed.data_ptr(), rgb.data_ptr())
        out.append((rgb.cpu().numpy().reshape(height, width, 3), err.cpu().numpy().reshape(height, width, 3),
                    mot.cpu().numpy().reshape(height, width, 3), took))
        prev_cam = cam
    return out


@pytest.mark.parametrize("denoise", [False, True])
@pytest.mark.parametrize("name", ["shirley", "cornell"])
def test_every_frame_is_the_chain_made_by_hand(P, torch, cases, name, denoise):
    import camera_pose_support as S
    c = cases[name]
    view, poses = S.cam4_of(c["desc"]), _poses(c["lens"][1])
    g = _scene(P, c)
    want = _by_hand(P, torch, g, view, poses, denoise)
    g.close()
    g = _scene(P, c)
    for f, pose in enumerate(poses):
        g.set_camera_pose(*pose)
        rgb, err, mot, took, st = g.render_temporal(W, H, N, DEPTH, (f * K) % N, K, denoise=True if denoise else None, want_err=True,
                                                    want_motion=True)
        for got, ref, what in ((rgb, want[f][0], "image"), (err, want[f][1], "error"), (mot, want[f][2], "motion")):
            assert np.array_equal(bits(got), bits(ref)), f"{name} frame {f}: the {what} differs"
        assert took == want[f][3] and st["samples"] == W * H * K
        if f == 0:
            assert took == 0 and not mot.any()  # the first frame of a sequence has no history
        else:
            assert took >= W * H // 2, (f, took)  # and the later ones mostly do: the comparison is not vacuous
    assert float(rgb.max()) > 0.0
    g.close()


def test_what_drops_the_history_and_what_does_not(P, cases):
    c = cases["shirley"]
    g = _scene(P, c)
    pose = _poses(c["lens"][1])[1]
    g.set_camera_pose(*pose)
    frame = lambda first, w=W, h=H: g.render_temporal(w, h, N, DEPTH, first, K, want_motion=True)  # noqa: E731
    assert frame(0)[3] == 0
    rgb1, _, mot, took, _ = frame(K)
    assert took > W * H // 2 and np.abs(mot[..., :2]).max() <= 1e-9  # a still camera: every pixel onto itself
    g.set_lighting(1)  # sticky state that is not the history's business: nothing but a reset or another size drops it
    g.set_lighting(0)
    assert frame(2 * K)[3] > W * H // 2
    g.temporal_reset()
    assert frame(0)[3] == 0
    again = frame(K)  # slice K onto slice 0 once more: the same inputs, the same bits
    assert again[3] == took and np.array_equal(bits(again[0]), bits(rgb1))
    assert frame(K, 32, 24)[3] == 0      # another size: dropped
    assert frame(2 * K, 32, 24)[3] > 0
    assert frame(0)[3] == 0              # and back
    # a refused call leaves the history as it was
    with pytest.raises(P.PtxError):
        g.render_temporal(W, H, N, DEPTH, N - 2, K)  # a range outside [0, N)
    assert frame(K)[3] == took
    g.close()


def test_the_same_slice_under_a_still_camera_gains_nothing(P, cases):
    """what the header says about advancing pass_first: the history and the frame are then the same numbers"""
    g = _scene(P, cases["shirley"])
    a = g.render_temporal(W, H, N, DEPTH, 0, K)
    b = g.render_temporal(W, H, N, DEPTH, 0, K)
    assert b[3] > W * H // 2
    # with history: H1 is the pixel's own mean (its neighbours' taps weigh 1e-16), blended with that same mean; without: the mean
    assert np.abs(b[0] - a[0]).max() <= 1e-12
    c = g.render_temporal(W, H, N, DEPTH, K, K)
    assert np.abs(c[0] - a[0]).max() > 1e-3  # another slice: other samples
    g.close()


def test_refusals(P, cases):
    c = cases["shirley"]
    g = _scene(P, c)
    g.set_lens(*c["lens"])
    p, t, out = P.render_params(W, H, N, DEPTH), P.temporal_defaults(), np.zeros((H, W, 3))
    from path_tracer_ocaml_amd import abi
    call = lambda first, count, params=p: P.lib().ptx_render_temporal(g._h, C.byref(params), C.byref(t), None, first, count,  # noqa: E731
                                                                       out.ctypes.data_as(abi.c_double_p), None, None, None, None)
    assert call(0, K) == PTX_ERR_STATE and "lens" in P.last_error()
    g.set_lens(0.0, 1.0)
    assert call(0, K) == 0
    assert call(0, 1) == PTX_ERR_ARG and call(N - 2, K) == PTX_ERR_ARG and call(-1, K) == PTX_ERR_ARG
    for field, v in (("n_gpus", 2), ("band_step", 2)):
        bad = P.render_params(W, H, N, DEPTH)
        setattr(bad, field, v)
        assert call(0, K, bad) == PTX_ERR_ARG, field
    t.min_weight = 1.0
    assert call(0, K) == PTX_ERR_ARG and "min_weight" in P.last_error()
    g.close()


def test_a_running_render_refuses_a_temporal_frame(P, cases):
    g = _scene(P, cases["shirley"])
    seen = []

    def on_update(passes_done, rel_err, rgb, err):
        try:
            g.render_temporal(W, H, N, DEPTH, 0, K)
        except P.PtxError as e:
            seen.append(str(e))
        try:
            g.temporal_reset()
        except P.PtxError as e:
            seen.append(str(e))
        return 1

    g.render_progressive(W, H, N, DEPTH, 4, on_update=on_update)
    assert len(seen) == 2 and all(f"({PTX_ERR_STATE})" in m for m in seen), seen
    g.close()


def test_a_pose_off_scene_is_the_identity_poses_camera(P, torch, cases):
    import camera_pose_support as S
    c = cases["shirley"]
    view = S.cam4_of(c["desc"])
    g = _scene(P, c)
    want = _by_hand(P, torch, g, view, [None, None], False)
    g.close()
    g = _scene(P, c)
    assert g.camera_pose is None
    for f in range(2):
        rgb, err, mot, took, _ = g.render_temporal(W, H, N, DEPTH, f * K, K, want_err=True, want_motion=True)
        assert np.array_equal(bits(rgb), bits(want[f][0])) and np.array_equal(bits(err), bits(want[f][1]))
        assert np.array_equal(bits(mot), bits(want[f][2])) and took == want[f][3]
    assert took > W * H // 2
    g.close()


def test_a_plain_render_is_untouched_by_a_temporal_frame(P, cases):
    g = _scene(P, cases["cornell"])
    before, _ = g.render(W, H, N, DEPTH)
    g.render_temporal(W, H, N, DEPTH, 0, K)
    g.render_temporal(W, H, N, DEPTH, K, K, denoise=True)
    after, _ = g.render(W, H, N, DEPTH)
    assert np.array_equal(bits(before), bits(after)) and float(before.max()) > 0.0
    g.close()
