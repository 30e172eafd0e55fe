"""ptx_render_rays / ptx_render_rays_device on the GPU (include/ptx.h, "radiance along rays the caller owns").

* per-ray radiance (one ray per bin onto zeros) is the restatement tests/c/rays_oracle.c bit for bit, compared as 0.0 + x on both
  sides: six scenes, every lighting mode each lists, depths 0 / 1 / 4, with the fused bounce kernel and under PTX_FUSED=0, on about
  250 rays per scene -- camera rays, rays leaving surfaces, rays from inside the glass, below the ground and far outside the tree,
  axis-parallel directions with signed zeros, directions of length 1e-3 .. 1e3 under PTX_RAYS_NORMALIZE -- at offsets 0, i,
  repeated values and 2^31 - 2;
* the rays ptx_camera_rays returns for all samples of a frame, at the offsets those samples have, give ptx_trace_samples' values bit
  for bit under a pinhole, a lens, a pose and both, with the same segment and work counters; sphere-light sampling is covered here;
* bins: sums and squares are the numpy left fold of the per-ray values at sizes around a wave and a block, onto zeros and onto
  what the buffers held, with bins that straddle the batches PTX_RAYS_BATCH forces, and twice the same bits;
* one bad ray of each kind hidden at the end of 1000 is refused with its index in the message and the sums untouched.

Without the feature there is no such entry point: every test here fails.
"""
import ctypes as C

import numpy as np
import pytest

import rays_support as RS
from rays_support import bits

pytestmark = pytest.mark.gpu
W, H, SPP = RS.W, RS.H, RS.SPP
PTX_ERR_ARG, PTX_ERR_STATE = -1, -3


@pytest.fixture(scope="module")
def P():
    import path_tracer_ocaml_amd as P
    assert P.lib().ptx_device_count() >= 1, P.last_error()
    return P


@pytest.fixture(scope="module")
def torch():
    return pytest.importorskip("torch")


def plus0(a):
    return bits(0.0 + RS.f64(a))


# ------------------------------------------------------------------------------------------------ 1. the restatement
@pytest.mark.parametrize("fused", [None, "0"])
@pytest.mark.parametrize("name", list(RS.CASES))
def test_rays_equal_the_restatement(P, oracle, monkeypatch, name, fused):
    if fused is not None:
        monkeypatch.setenv("PTX_FUSED", fused)  # read when the scene is created: k_trace + k_shade_pool instead of k_bounce
    c = RS.case(name, oracle)
    fam = RS.ray_families(c)
    rays, offsets, scaled = fam["rays"], fam["offsets"], fam["scaled"]
    lit = False
    for mode in RS.CASES[name]:
        g = RS.LS.gpu_scene(P, c, mode, lens=False)
        for depth in RS.DEPTHS:
            want, segments = c["rays_ref"].trace_rays(rays, offsets, depth, None, c["images"], c["env"], mode, c["sampling"])
            got, sq, st = g.render_rays(rays[:, :3], rays[:, 3:], offsets, max_bounces=depth, want_sq=True, count_work=True)
            nbad = int((plus0(got) != plus0(want)).any(axis=1).sum())
            assert nbad == 0, f"{name} mode {mode} depth {depth} fused {fused}: {nbad} of {len(rays)} rays differ"
            assert np.array_equal(bits(sq), bits(0.0 + got * got))
            assert st["samples"] == len(rays) and st["segments"] == segments
            want, _ = c["rays_ref"].trace_rays(scaled, offsets, depth, None, c["images"], c["env"], mode, c["sampling"], normalize=True)
            got, _, _ = g.render_rays(scaled[:, :3], scaled[:, 3:], offsets, max_bounces=depth, normalize=True)
            nbad = int((plus0(got) != plus0(want)).any(axis=1).sum())
            assert nbad == 0, f"{name} mode {mode} depth {depth} fused {fused}, normalised: {nbad} of {len(rays)} rays differ"
            lit = lit or float(want.max()) > 0.0
        g.close()
    assert lit


# ------------------------------------------------------------------------------------------------ 2. ptx_trace_samples
def _check_against_trace_samples(g, depth, label):
    xs, ys, ps = RS.all_samples()
    offsets = RS.frame_offsets()
    o, d = g.camera_rays(W, H, SPP, depth, xs, ys, ps)
    want, wst = g.trace_samples(W, H, SPP, depth, xs, ys, ps, count_work=True)
    got, _, st = g.render_rays(o, d, offsets, max_bounces=depth, count_work=True)
    nbad = int((bits(got) != bits(want)).any(axis=1).sum())
    assert nbad == 0, f"{label} depth {depth}: {nbad} of {len(xs)} samples differ"
    keys = ("samples", "segments", "nodes_tested", "prims_tested", "floor_tested")
    print(label, depth, {k: (st[k], wst[k]) for k in keys})
    assert [st[k] for k in keys] == [wst[k] for k in keys], label
    return want


@pytest.mark.parametrize("state", ["pinhole", "lens", "pose", "pose_lens"])
@pytest.mark.parametrize("name", list(RS.CASES))
def test_camera_rays_give_what_trace_samples_gives(P, oracle, name, state):
    c = RS.case(name, oracle)
    pose = c["poses"]["oblique"] if state.startswith("pose") else None
    g = RS.CS.gpu_scene(P, c, pose, RS.CASES[name][-1], lens=state.endswith("lens"))
    seen = 0.0
    for depth in RS.DEPTHS:
        seen = max(seen, float(_check_against_trace_samples(g, depth, f"{name} {state}").max()))
    assert seen > 0.0
    g.close()


def test_sphere_light_sampling_is_part_of_the_shading_state(P, oracle):
    import spherelight_support as SS
    g = SS.gpu_scene(P, "shirley", on=True, mode=2, w=W, h=H)
    on = _check_against_trace_samples(g, 4, "sphere lights on")
    g.close()
    g = SS.gpu_scene(P, "shirley", on=False, mode=1, w=W, h=H)  # (sampled lighting has nothing else to sample in this scene)
    off = _check_against_trace_samples(g, 4, "sphere lights off, path order")
    assert (bits(on) != bits(off)).any()
    g.close()


# ------------------------------------------------------------------------------------------------ 3. the folds
FOLD_N = (1, 63, 64, 65, 255, 256, 257, 999, 1000)


@pytest.fixture(scope="module")
def fold(P, oracle):
    """1000 camera rays of a 40 x 25 frame of the Shirley scene, their offsets and their per-ray radiance at depth 4"""
    c = RS.case("shirley", oracle)
    g = RS.LS.gpu_scene(P, c, 0, lens=False)
    xs, ys, ps = RS.all_samples(40, 25, 1)
    o, d = g.camera_rays(40, 25, 1, 4, xs, ys, ps)
    offsets = RS.frame_offsets(40, 25, 1)
    per_ray, _, _ = g.render_rays(o, d, offsets, max_bounces=4)
    assert float(per_ray.max()) > 0.0 and len(np.unique(bits(per_ray)[:, 0])) > 100
    yield g, o, d, offsets, per_ray
    g.close()


def _bins(n):
    return sorted({m for m in (1, 3, 64, 100, n) if n % m == 0})


@pytest.mark.parametrize("batch", [None, "192"])
def test_bins_are_the_left_fold_of_the_per_ray_values(fold, monkeypatch, batch):
    g, o, d, offsets, per_ray = fold
    if batch is not None:
        monkeypatch.setenv("PTX_RAYS_BATCH", batch)  # 1000 rays: six batches, and bins of 100 straddle them
    for n in FOLD_N:
        for m in _bins(n):
            got, sq, st = g.render_rays(o[:n], d[:n], offsets[:n], max_bounces=4, rays_per_bin=m, want_sq=True)
            assert got.shape == (n // m, 3) and st["samples"] == n
            assert np.array_equal(bits(got), bits(RS.left_fold(per_ray[:n], m))), (n, m, batch)
            assert np.array_equal(bits(sq), bits(RS.left_fold(per_ray[:n], m, squares=True))), (n, m, batch)


@pytest.mark.parametrize("batch", [None, "192"])
def test_the_device_call_continues_from_what_the_buffers_hold(P, torch, fold, monkeypatch, batch):
    g, o, d, offsets, per_ray = fold
    if batch is not None:
        monkeypatch.setenv("PTX_RAYS_BATCH", batch)
    d_o, d_d = torch.tensor(o, device="cuda:0"), torch.tensor(d, device="cuda:0")
    d_off = torch.tensor(offsets, device="cuda:0")
    rng = np.random.default_rng(11)
    for n, m in ((1000, 100), (1000, 1), (999, 3), (257, 257), (64, 64)):
        init, init_sq = rng.random((n // m, 3)), rng.random((n // m, 3))
        runs = []
        for _ in range(2):
            s, q = torch.tensor(init, device="cuda:0"), torch.tensor(init_sq, device="cuda:0")
            st = g.render_rays_device(n, d_o.data_ptr(), d_d.data_ptr(), s.data_ptr(), d_off.data_ptr(), q.data_ptr(), max_bounces=4,
                                      rays_per_bin=m)
            assert st["samples"] == n
            runs.append((s.cpu().numpy(), q.cpu().numpy()))
        assert np.array_equal(bits(runs[0][0]), bits(RS.left_fold(per_ray[:n], m, init))), (n, m, batch)
        assert np.array_equal(bits(runs[0][1]), bits(RS.left_fold(per_ray[:n], m, init_sq, squares=True))), (n, m, batch)
        assert np.array_equal(bits(runs[0][0]), bits(runs[1][0])) and np.array_equal(bits(runs[0][1]), bits(runs[1][1]))
    # without squares, on a stream of the caller's, and with NULL offsets (offset i = i: the frame's own at one pass per pixel)
    stream = torch.cuda.Stream()
    s = torch.zeros((10, 3), dtype=torch.float64, device="cuda:0")
    g.render_rays_device(1000, d_o.data_ptr(), d_d.data_ptr(), s.data_ptr(), max_bounces=4, rays_per_bin=100, stream=stream.cuda_stream)
    assert np.array_equal(bits(s.cpu().numpy()), bits(RS.left_fold(per_ray, 100)))


def test_no_rays_is_no_work(P, fold):
    g, o, d, offsets, _ = fold
    got, _, st = g.render_rays(o[:0], d[:0], max_bounces=4)
    assert got.shape == (0, 3) and st["samples"] == 0


# ------------------------------------------------------------------------------------------------ 4. refusals
@pytest.mark.parametrize("kind, words", [("nan_origin", "not finite"), ("inf_origin", "not finite"), ("nan_direction", "not finite"),
                                         ("inf_direction", "not finite"), ("zero_direction", "direction (0, 0, 0)"),
                                         ("negative_offset", "sampler offset -1"), ("min_offset", "sampler offset -2147483648")])
def test_one_bad_ray_at_the_end_is_refused_by_its_index(P, torch, fold, kind, words):
    g, o, d, offsets, _ = fold
    o, d, offsets = o.copy(), d.copy(), offsets.copy()
    at = len(o) - 1
    if kind == "nan_origin":
        o[at, 1] = np.nan
    elif kind == "inf_origin":
        o[at, 2] = -np.inf
    elif kind == "nan_direction":
        d[at, 0] = np.nan
    elif kind == "inf_direction":
        d[at, 2] = np.inf
    elif kind == "zero_direction":
        d[at] = (0.0, -0.0, 0.0)
    elif kind == "negative_offset":
        offsets[at] = -1
    elif kind == "min_offset":
        offsets[at] = -2**31
    d_o, d_d, d_off = (torch.tensor(a, device="cuda:0") for a in (o, d, offsets))
    s = torch.full((10, 3), 7.0, dtype=torch.float64, device="cuda:0")
    q = torch.full((10, 3), 5.0, dtype=torch.float64, device="cuda:0")
    p = P.abi.rays_params(4, 100)
    rc = P.lib().ptx_render_rays_device(g._h, C.byref(p), 1000, d_o.data_ptr(), d_d.data_ptr(), d_off.data_ptr(), s.data_ptr(), q.data_ptr(),
                                        None, None)
    msg = P.last_error()
    assert rc == PTX_ERR_ARG and msg.startswith(f"ray {at} ") and words in msg, msg
    assert (s.cpu().numpy() == 7.0).all() and (q.cpu().numpy() == 5.0).all()  # the sums are left untouched
    with pytest.raises(P.PtxError, match=f"ray {at} "):
        g.render_rays(o, d, offsets, max_bounces=4)


def test_the_message_names_the_lowest_bad_ray_and_the_largest_offset_is_accepted(P, fold):
    g, o, d, offsets, _ = fold
    o, d, offsets = o.copy(), d.copy(), offsets.copy()
    offsets[3] = RS.MAX_OFFSET
    g.render_rays(o, d, offsets, max_bounces=1)
    d[700] = 0.0
    o[401, 0] = np.nan
    offsets[998] = -5
    with pytest.raises(P.PtxError, match="ray 401 "):
        g.render_rays(o, d, offsets, max_bounces=1)


def test_a_call_from_a_callback_of_a_running_render_is_refused(P, oracle, fold):
    g, o, d, offsets, _ = fold
    seen = []
    out = np.zeros((4, 3))
    p = P.abi.rays_params(2)

    def progress(n):
        dp = P.abi.c_double_p
        seen.append(P.lib().ptx_render_rays(g._h, C.byref(p), 4, o.ctypes.data_as(dp), d.ctypes.data_as(dp), None, out.ctypes.data_as(dp),
                                            None, None))
    g.render(64, 32, 2, 4, progress=progress)
    assert seen and set(seen) == {PTX_ERR_STATE} and "while a render runs" in P.last_error()
    assert not out.any()
