"""The camera shutter on the GPU (include/ptx.h, ptx_scene_set_camera_shutter) against the numpy rule (tests/shutter_reference.py) and
the restatement tests/c/shutter_oracle.c, at 13 x 11 (two tile columns and two tile rows, both ragged), spp 4.

* ptx_camera_rays is the numpy rule bit for bit for every sample of the frame, with t taken from ptx_lds_sample at dimension d - 1:
  an oblique pose with a shutter that translates and turns, a pure turn, a pure translation, the pose off, a lens, LATLONG;
* per-sample radiance (ptx_trace_samples) at depths 0, 1 and 4 is the restatement's bit for bit on the six scenes of the pose's tests,
  with equal segment counts, on the fused and on the two-kernel schedule (PTX_FUSED=0);
* raw sums (13 x 11 and 1 x 1: the generator's order, ids and holes), bands, slices of passes, a pixel list, the progressive, adaptive
  and denoised drivers, the display form, the feature buffers and two aliased replicas all give the per-sample values;
* with the shutter off again the handle renders its earlier image and launches its earlier kernels; a lens switched on and off under
  a shutter moves the lens pair; every refusal leaves its outputs untouched.

Without the feature there is no such setter: every test here fails.
"""
import ctypes as C

import numpy as np
import pytest

import shutter_reference as SR
import shutter_support as S

pytestmark = pytest.mark.gpu
bits = S.bits
W, H, SPP = S.W, S.H, S.SPP
STATES = ["both", "turn", "move", "pose_off", "lens", "latlong"]
PTX_ERR_ARG, PTX_ERR_STATE = -1, -3
WAY_OUT = "ptx_scene_set_camera_shutter(scene, NULL, NULL, 0) first"


@pytest.fixture(scope="module")
def P():
    import path_tracer_ocaml_amd as P
    assert P.lib().ptx_device_count() >= 1, P.last_error()
    return P


@pytest.fixture(scope="module")
def torch():
    return pytest.importorskip("torch")


def _raw(torch, g, params, rows=None):
    buf = torch.zeros((rows if rows is not None else params.height, params.width, 3), dtype=torch.float64, device="cuda:0")
    st = g.render_raw_device(params, buf.data_ptr())
    return buf.cpu().numpy(), st


def _times(P, c, state, depth, w, h, spp, xs, ys, ps):
    """the samples' times as the library's own sampler gives them: dimension d - 1 of the d-dimensional sequence"""
    d = SR.dimension(depth, c["lens"] if state.lens else None)
    off = (ys.astype(np.int64) * w + xs + ps.astype(np.int64) * spp).astype(np.int32)
    return P.lds_sample(d, off, np.full(len(off), d - 1, dtype=np.int32))


# ------------------------------------------------------------------------------------------------ the rays
@pytest.mark.parametrize("state", STATES)
def test_camera_rays_equal_the_numpy_rule(P, oracle, state):
    c = S.case("shirley", oracle)
    st = c["states"][state]
    g = S.gpu_scene(P, c, st)
    for (w, h), depth in (((W, H), 4), ((W, H), 0), ((1, 1), 1), ((64, 8), 4)):
        xs, ys, ps = S.all_samples(w, h, SPP)
        o, d = g.camera_rays(w, h, SPP, depth, xs, ys, ps)
        t = _times(P, c, st, depth, w, h, SPP, xs, ys, ps)
        assert (t >= 0.0).all() and (t < 1.0).all() and (len(t) == 4 or len(np.unique(t)) > len(t) // 4)
        want = S.numpy_rays(oracle, c, st, w, h, SPP, depth, xs, ys, ps, t=t)
        assert np.array_equal(bits(o), bits(want[:, :3])) and np.array_equal(bits(d), bits(want[:, 3:])), (w, h, depth)
        # and the sampler restated on the CPU gives the same times: the whole ray from the header's text alone
        assert np.array_equal(bits(np.concatenate([o, d], axis=1)), bits(S.numpy_rays(oracle, c, st, w, h, SPP, depth, xs, ys, ps)))
    g.close()


def test_a_lens_switched_on_and_off_under_a_shutter_moves_the_lens_pair(P, oracle):
    """shutter on, then the lens on: d grows by two, t stays last and the pair sits at d - 3 and d - 2; lens off again: the first rays"""
    c = S.case("shirley", oracle)
    no_lens, lens = c["states"]["both"], c["states"]["lens"]
    g = S.gpu_scene(P, c, no_lens)
    xs, ys, ps = S.all_samples()
    first = np.concatenate(g.camera_rays(W, H, SPP, 4, xs, ys, ps), axis=1)
    assert np.array_equal(bits(first), bits(S.numpy_rays(oracle, c, no_lens, W, H, SPP, 4, xs, ys, ps)))
    g.set_lens(*c["lens"])
    with_lens = np.concatenate(g.camera_rays(W, H, SPP, 4, xs, ys, ps), axis=1)
    assert np.array_equal(bits(with_lens), bits(S.numpy_rays(oracle, c, lens, W, H, SPP, 4, xs, ys, ps)))
    assert (bits(with_lens) != bits(first)).any(axis=1).all()
    g.set_lens(0.0, 1.0)
    assert np.array_equal(bits(np.concatenate(g.camera_rays(W, H, SPP, 4, xs, ys, ps), axis=1)), bits(first))
    g.close()


# ------------------------------------------------------------------------------------------------ per sample
def _samples_equal_the_restatement(P, oracle, name, states):
    c = S.case(name, oracle)
    mode = S.CASES[name][-1]
    xs, ys, ps = S.all_samples()
    g = S.gpu_scene(P, c, None, mode)
    for state in states:
        st = c["states"][state]
        st.set_on(g, c)
        for depth in S.DEPTHS:
            got, stats = g.trace_samples(W, H, SPP, depth, xs, ys, ps, count_work=True)
            want, segments = S.restated(c, st, depth, mode)
            nbad = int((bits(got) != bits(want)).any(axis=1).sum())
            assert nbad == 0, f"{name} {state} mode {mode} depth {depth}: {nbad} of {len(xs)} samples differ"
            assert stats["segments"] == segments and stats["carry_launches"] == 0 and stats["solo_launches"] == 0
            if c["lds"] is not None:
                assert stats["traversal_in_lds"] == bool(c["lds"]), name
        assert float(want.max()) > 0.0, state
    g.close()


@pytest.mark.parametrize("name", list(S.CASES))
def test_samples_equal_the_restatement(P, oracle, name):
    _samples_equal_the_restatement(P, oracle, name, STATES)


@pytest.mark.parametrize("name", ["shirley", "cornell"])
def test_samples_equal_the_restatement_on_the_two_kernel_schedule(P, oracle, monkeypatch, name):
    monkeypatch.setenv("PTX_FUSED", "0")  # read when the scene is created: k_trace + k_shade_pool
    _samples_equal_the_restatement(P, oracle, name, ["both", "lens", "latlong"])


# ------------------------------------------------------------------------------------------------ the drivers
@pytest.fixture(scope="module", params=[("shirley", "both"), ("shirley", "lens"), ("cornell", "latlong"), ("mesh", "pose_off"),
                                        ("image", "turn"), ("envlight", "move")], ids=lambda p: "-".join(p))
def frame(request, P, oracle):
    """a 13 x 11 frame of a case under a camera state: the scene, the restated per-sample values at depth 4 and its image"""
    name, state = request.param
    c = S.case(name, oracle)
    mode = S.CASES[name][-1]
    st = c["states"][state]
    g = S.gpu_scene(P, c, st, mode)
    samples, segments = S.restated(c, st, 4, mode)
    rgb, _ = g.render(W, H, SPP, 4, passes_per_batch=2)
    yield name, c, st, g, samples, segments, rgb.copy()
    g.close()


def test_raw_sums_are_the_samples_in_pass_order(P, torch, frame):
    name, c, st, g, samples, segments, _ = frame
    want = S.pass_order_sums(samples, W, H, SPP)
    for ppb in (1, 2, 0):
        raw, stats = _raw(torch, g, P.render_params(W, H, SPP, 4, passes_per_batch=ppb, count_work=True))
        assert np.array_equal(bits(raw), bits(want)), (name, ppb)
        assert stats["segments"] == segments
        assert stats["carry_launches"] == 0 and stats["solo_launches"] == 0 and stats["lds_oct_launches"] == 0
    timed, stats = _raw(torch, g, P.render_params(W, H, SPP, 4, passes_per_batch=1, time_kernels=True))
    assert stats["kernel_launches"]["generate"] == SPP and np.array_equal(bits(timed), bits(want))
    assert g.tile_list_stats()["list_launches"] == 0
    buf = torch.zeros((H, W, 3), dtype=torch.float64, device="cuda:0")
    g.render_raw_device(P.render_params(W, H, SPP, 4, passes_per_batch=1, asynchronous=True), buf.data_ptr())
    torch.cuda.synchronize()
    assert np.array_equal(bits(buf.cpu().numpy()), bits(want)), name
    # slices of passes onto the same buffer
    buf = torch.zeros((H, W, 3), dtype=torch.float64, device="cuda:0")
    params = P.render_params(W, H, SPP, 4)
    g.render_passes_device(params, 0, 3, buf.data_ptr())
    g.render_passes_device(params, 3, 1, buf.data_ptr())
    assert np.array_equal(bits(buf.cpu().numpy()), bits(want)), name


def test_a_one_pixel_frame_is_its_samples(P, torch, frame):
    """1 x 1: one valid lane in one tile, 63 holes"""
    name, c, st, g, _, _, _ = frame
    xs, ys, ps = S.all_samples(1, 1, SPP)
    want, _ = S.restated(c, st, 4, S.CASES[name][-1], width=1, height=1)
    raw, _ = _raw(torch, g, P.render_params(1, 1, SPP, 4))
    assert np.array_equal(bits(raw), bits(S.pass_order_sums(want, 1, 1, SPP))), name


def test_the_frame_is_the_film_of_those_sums_and_every_driver_renders_it(P, torch, frame):
    name, c, st, g, samples, _, rgb = frame
    sums = torch.tensor(S.pass_order_sums(samples, W, H, SPP), device="cuda:0")
    out = torch.zeros_like(sums)
    P.film_resolve_device(0, W, H, SPP, sums.data_ptr(), out.data_ptr())
    assert np.array_equal(bits(out.cpu().numpy()), bits(rgb)), name
    got, _, done, _ = g.render_progressive(W, H, SPP, 4, passes_per_update=3)
    assert done == SPP and np.array_equal(bits(got), bits(rgb)), name
    got, _, passes, _ = g.render_adaptive(W, H, SPP, 4, 0.0, min_passes=2, passes_per_round=1)
    assert (passes == SPP).all() and np.array_equal(bits(got), bits(rgb)), name
    got, _, _, done, _ = g.render_denoised(W, H, SPP, 4, passes_per_update=3, denoise={"levels": 0})
    assert done == SPP and np.array_equal(bits(got), bits(rgb)), name
    # the display form: the bytes of that image
    pixels, _ = g.render_display(W, H, SPP, 4, passes_per_batch=2)
    assert np.array_equal(pixels, P.display_apply(rgb)), name


def test_a_ragged_pixel_list_gives_those_pixels_sums(P, torch, frame):
    name, c, st, g, samples, _, _ = frame
    want = S.pass_order_sums(samples, W, H, SPP).reshape(-1, 3)
    pix = np.random.default_rng(9).choice(W * H, 37, replace=False).astype(np.int32)  # no multiple of a wave, unordered
    d_pix = torch.tensor(pix, device="cuda:0")
    raw = torch.zeros((H, W, 3), dtype=torch.float64, device="cuda:0")
    stats = g.render_pixels_device(P.render_params(W, H, SPP, 4, passes_per_batch=2), 0, SPP, d_pix.data_ptr(), len(pix), raw.data_ptr())
    raw = raw.cpu().numpy().reshape(-1, 3)
    assert stats["samples"] == len(pix) * SPP
    assert np.array_equal(bits(raw[pix]), bits(want[pix])), name
    assert (raw[np.setdiff1d(np.arange(W * H), pix)] == 0.0).all()


def test_features_are_the_first_hits_of_the_shutter_rays(P, torch, frame):
    name, c, st, g, _, _, _ = frame
    xs, ys, ps = S.all_samples()
    want = c["sref"].first_hits(c, st, W, H, SPP, 4, xs, ys, ps).reshape(H * W, SPP, 8)
    sums = np.zeros((H * W, 8))
    for k in range(SPP):
        sums = sums + want[:, k]
    feat = torch.zeros((H, W, 8), dtype=torch.float64, device="cuda:0")
    params = P.render_params(W, H, SPP, 4, passes_per_batch=2)
    g.render_features_device(params, 0, 3, feat.data_ptr())
    g.render_features_device(params, 3, 1, feat.data_ptr())
    got = feat.cpu().numpy().reshape(-1, 8)
    assert np.array_equal(got[:, 7], sums[:, 7]) and 0 < sums[:, 7].sum(), name
    assert np.array_equal(bits(got[:, 6]), bits(sums[:, 6])), "depth"
    assert np.array_equal(bits(got[:, :3]), bits(sums[:, :3])), "albedo"
    assert np.array_equal(bits(got[:, 3:6]), bits(sums[:, 3:6])), "normal"


@pytest.mark.parametrize("ranks", [2, 3])
def test_bands_are_the_rows_of_the_frame(P, oracle, torch, ranks):
    w, h, depth = 13, 27, 4  # bands of 8 rows dealt to the ranks; the last band is ragged
    c = S.case("shirley", oracle, w, h)
    st = c["states"]["both"]
    g = S.gpu_scene(P, c, st)
    whole, _ = _raw(torch, g, P.render_params(w, h, SPP, depth, passes_per_batch=1))
    want, _ = S.restated(c, st, depth, width=w, height=h)
    assert np.array_equal(bits(whole), bits(S.pass_order_sums(want, w, h, SPP)))
    seen = []
    for first in range(ranks):
        params = P.render_params(w, h, SPP, depth, passes_per_batch=1, band_rows=8, band_first=first, band_step=ranks)
        rows = P.lib().ptx_local_rows(C.byref(params))
        band, _ = _raw(torch, g, params, rows)
        global_rows = [P.lib().ptx_global_row(C.byref(params), k) for k in range(rows)]
        assert np.array_equal(bits(band), bits(whole[global_rows])), first
        seen += global_rows
    assert sorted(seen) == list(range(h))
    g.close()


def test_replicas_carry_the_shutter(P, oracle, monkeypatch):
    c = S.case("shirley", oracle)
    st = c["states"]["both"]
    g = S.gpu_scene(P, c, st)
    rgb, _ = g.render(W, H, SPP, 4)
    monkeypatch.setenv("PTX_MULTI_ALIAS", "1")  # test hook: replicas may share a device
    r = g.replicate(0)
    for got, want in zip(r.camera_shutter, g.camera_shutter):
        assert np.array_equal(got, want)
    assert np.array_equal(g.camera_shutter[0], st.shutter[0])
    got, _ = P.render_multi([g, r], W, H, SPP, 4)
    assert np.array_equal(bits(got), bits(rgb))
    # a replica with another shutter, or with none, is not a replica of the same picture
    r.set_camera_shutter(st.shutter[0] * 2.0, st.shutter[1], st.shutter[2])
    with pytest.raises(P.PtxError, match="does not carry the camera shutter"):
        P.render_multi([g, r], W, H, SPP, 4)
    r.set_camera_shutter()
    with pytest.raises(P.PtxError, match="does not carry the camera shutter"):
        P.render_multi([g, r], W, H, SPP, 4)
    r.close()
    got, _ = g.render(W, H, SPP, 4, n_gpus=2)  # the replicas a scene owns follow the setter
    assert np.array_equal(bits(got), bits(rgb))
    c["states"]["turn"].set_on(g, c)
    one, _ = g.render(W, H, SPP, 4)
    two, _ = g.render(W, H, SPP, 4, n_gpus=2)
    assert np.array_equal(bits(one), bits(two)) and not np.array_equal(bits(one), bits(rgb))
    g.close()


# ------------------------------------------------------------------------------------------------ on and off
@pytest.mark.parametrize("name, pose, lens", [("shirley", None, False), ("shirley", "oblique", False), ("shirley", "oblique", True),
                                              ("mesh", None, False)])
def test_the_shutter_off_again_is_the_handle_as_it_was(P, oracle, torch, name, pose, lens):
    """the image bit for bit, the work counters, and the kernels launched: what they were before the shutter was ever set"""
    c = S.case(name, oracle)
    g = S.LS.gpu_scene(P, c, 0, lens=lens)
    if pose:
        c["poses"][pose].set_on(g)
    params, counting = P.render_params(W, H, SPP, 4), P.render_params(W, H, SPP, 4, count_work=True)
    g.clear_launched_kernels()
    home, _ = _raw(torch, g, params)
    _, before = _raw(torch, g, counting)
    kernels = g.launched_kernels()
    lists_before = g.tile_list_stats()
    assert kernels and float(home.max()) > 0.0
    T, k, A = c["states"]["both"].shutter
    g.set_camera_shutter(T, k, A)
    moved, st = _raw(torch, g, counting)
    assert not np.array_equal(bits(moved), bits(home))
    assert st["carry_launches"] == 0 and st["lds_oct_launches"] == 0 and st["solo_launches"] == 0 and st["primary_lane_walks"] == 0
    assert g.tile_list_stats() == lists_before  # a shutter render builds and scans no tile lists
    g.set_camera_shutter(np.zeros(3), np.zeros(3), 0.0)  # no motion is still ON: another alpha table, another picture
    still, _ = _raw(torch, g, params)
    assert not np.array_equal(bits(still), bits(home))
    g.set_camera_shutter(None)
    g.clear_launched_kernels()
    again, _ = _raw(torch, g, params)
    _, after = _raw(torch, g, counting)
    assert np.array_equal(bits(again), bits(home))
    assert g.launched_kernels() == kernels
    for key in ("carry_launches", "lds_oct_launches", "solo_launches", "primary_lane_walks", "segments"):
        assert after[key] == before[key], key
    g.close()


# ------------------------------------------------------------------------------------------------ refusals
def test_every_refusal_leaves_its_outputs_untouched(P, oracle):
    c = S.case("cornell", oracle)
    g = S.gpu_scene(P, c, c["states"]["pose_off"])  # (with a pose on, the pose's own refusal comes first)
    L = P.lib()
    ip, dp = P.abi.c_int32_p, P.abi.c_double_p
    out = np.full((H, W, 3), 7.0)
    with pytest.raises(P.PtxError) as e:
        g.render_temporal(W, H, 4, 4, 0, 4, out=out)
    assert "(-3)" in str(e.value) and WAY_OUT in str(e.value) and (out == 7.0).all()
    with pytest.raises(P.PtxError) as e:
        g.ppm_render(P.abi.ppm_params(W, H, iterations=1, photon_count=2000), oracle.lights_cornell(W, H))
    assert "(-3)" in str(e.value) and WAY_OUT in str(e.value)
    xs = np.zeros(4, dtype=np.int32)
    p = P.render_params(W, H, 4, 4)
    ray, attn, alive = np.full((4, 6), 7.0), np.full((4, 3), 7.0), np.full(4, 7, dtype=np.int32)
    L.ptx_debug_first_scatter.argtypes = [C.c_void_p, C.POINTER(P.abi.RenderParams), C.c_int64, ip, ip, ip, dp, dp, ip]
    rc = L.ptx_debug_first_scatter(g._h, C.byref(p), 4, xs.ctypes.data_as(ip), xs.ctypes.data_as(ip), xs.ctypes.data_as(ip),
                                   ray.ctypes.data_as(dp), attn.ctypes.data_as(dp), alive.ctypes.data_as(ip))
    assert rc == PTX_ERR_STATE and WAY_OUT in P.last_error()
    assert (ray == 7.0).all() and (attn == 7.0).all() and (alive == 7).all()
    # lens + shutter at depth 126: one dimension too many; 125 renders, and so does 126 without the lens
    g.set_lens(*c["lens"])
    rgb = np.full((1, 1, 3), 7.0)
    p126 = P.render_params(1, 1, 1, 126)
    assert L.ptx_render(g._h, C.byref(p126), rgb.ctypes.data_as(dp), None, None, None) == PTX_ERR_ARG
    assert "at most 125 bounces with a lens" in P.last_error() and (rgb == 7.0).all()
    o, d = np.full((1, 3), 7.0), np.full((1, 3), 7.0)
    assert L.ptx_camera_rays(g._h, C.byref(p126), 1, xs.ctypes.data_as(ip), xs.ctypes.data_as(ip), xs.ctypes.data_as(ip), o.ctypes.data_as(dp),
                             d.ctypes.data_as(dp)) == PTX_ERR_ARG
    assert (o == 7.0).all() and (d == 7.0).all()
    one = np.zeros(1, dtype=np.int32)
    st = S.State(None, lens=True, shutter=c["states"]["pose_off"].shutter)
    got = np.concatenate(g.camera_rays(1, 1, 1, 125, one, one, one), axis=1)  # d = 255: t at 254, the pair at 252 and 253
    assert np.array_equal(bits(got), bits(S.numpy_rays(oracle, c, st, 1, 1, 1, 125, one, one, one)))
    g.set_lens(0.0, 1.0)
    got = np.concatenate(g.camera_rays(1, 1, 1, 126, one, one, one), axis=1)  # d = 255 again
    assert np.array_equal(bits(got), bits(S.numpy_rays(oracle, c, c["states"]["pose_off"], 1, 1, 1, 126, one, one, one)))
    # the setter is refused while a render runs
    seen = []
    g.render(64, 32, 2, 4, progress=lambda n: seen.append(L.ptx_scene_set_camera_shutter(g._h, None, None, 0.0)))
    assert seen and set(seen) == {PTX_ERR_STATE} and "while a render runs" in P.last_error() and g.camera_shutter is not None
    g.close()
