"""The thin-lens camera on the GPU (include/ptx.h, ptx_scene_set_lens) against the restatement tests/c/lens_oracle.c.

* per-sample radiance (ptx_trace_samples) of every sample of a 13 x 11 frame, 3 passes, at depths 0, 1 and 4 is the restatement's bit
  for bit: Shirley Simd_leaf (LDS-resident: the scene that would otherwise take the shade-first order, the per-octant image and tile
  lists), Shirley Array_leaf, Cornell with its emitter in lighting modes 0, 1 and 2, a mesh walked from HBM / L2 behind its floor, a
  scene with image textures, a scene lit by a sampled environment;
* whole frames: the raw sums of three batches on two streams are the per-sample values summed in pass order; bands are the frame's
  rows; a counting render traces the restatement's segments, never takes the shade-first order, and generates once per batch;
* a lens set and switched off again leaves a scene that renders, and schedules, like one never touched;
* the drivers (progressive, denoised with no levels, adaptive with T = 0, a pixel list, two replicas) give the frame; the feature
  buffers show the first hit of the lens ray;
* ptx_ppm_render and ptx_debug_first_scatter refuse a scene whose lens is on.

tests/test_lens_reference.py asserts, on these very inputs, that the restatement's lens rays differ from the pinhole's on every sample
and the radiance on some: a GPU that ignored the lens cannot pass.
"""
import ctypes as C

import numpy as np
import pytest

import lens_support as S

pytestmark = pytest.mark.gpu
bits = S.bits
W, H, SPP = S.W, S.H, S.SPP


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


# ------------------------------------------------------------------------------------------------ per sample
@pytest.mark.parametrize("name, mode", [(n, m) for n, modes in S.CASES.items() for m in modes])
def test_samples_equal_the_restatement(P, oracle, name, mode):
    c = S.case(name, oracle)
    g = S.gpu_scene(P, c, mode)
    assert g.lens() == c["lens"]
    xs, ys, ps = S.all_samples()
    for depth in S.DEPTHS:
        got, st = g.trace_samples(W, H, SPP, depth, xs, ys, ps, count_work=True)
        want, segments = S.restated(c, depth, mode)
        nbad = int((bits(got) != bits(want)).any(axis=1).sum())
        assert nbad == 0, f"{name} mode {mode} depth {depth}: {nbad} of {len(xs)} samples differ"
        assert st["segments"] == segments and st["carry_launches"] == 0 and st["solo_launches"] == 0
        if c["lds"] is not None:
            assert st["traversal_in_lds"] == bool(c["lds"]), name
    assert float(want.max()) > 0.0
    g.close()


# ------------------------------------------------------------------------------------------------ whole frames
@pytest.mark.parametrize("name", ["shirley", "cornell", "mesh"])
def test_raw_sums_are_the_samples_in_pass_order(P, oracle, torch, name):
    """passes_per_batch = 1: three batches, both streams"""
    c = S.case(name, oracle)
    mode = S.CASES[name][-1]
    g = S.gpu_scene(P, c, mode)
    depth = 4
    raw, _ = _raw(torch, g, P.render_params(W, H, SPP, depth, passes_per_batch=1))
    want, segments = S.restated(c, depth, mode)
    assert np.array_equal(bits(raw), bits(S.pass_order_sums(want, W, H, SPP)))
    # counting: the restatement's segments, no shade-first launch; timed: one generate launch per batch
    _, st = _raw(torch, g, P.render_params(W, H, SPP, depth, passes_per_batch=1, count_work=True))
    assert st["segments"] == segments and st["carry_launches"] == 0 and st["primary_lane_walks"] == 0 and st["lds_oct_launches"] == 0
    timed, st = _raw(torch, g, P.render_params(W, H, SPP, depth, passes_per_batch=1, time_kernels=True))
    assert st["kernel_launches"]["generate"] == 3
    assert np.array_equal(bits(timed), bits(raw))
    assert g.tile_list_stats()["list_launches"] == 0
    g.close()


@pytest.mark.parametrize("name, knobs, two_kernels", [("shirley", {"PTX_FUSED": "0"}, True), ("shirley", {"PTX_FUSED": "1"}, False),
                                                      ("cornell", {"PTX_FUSED": "0"}, True), ("mesh", {"PTX_FUSED_GLOBAL": "0"}, True)])
def test_the_two_kernel_bounces_take_generated_rays_too(P, oracle, torch, monkeypatch, name, knobs, two_kernels):
    """k_trace + k_shade_pool behind k_generate_tiles (the knobs are read when the handle is created), and a frame queued with
    PTX_RENDER_ASYNC.  PTX_FUSED=1 keeps only the camera LAUNCH on the two kernels: a lens render has none, its bounce 0 is a queued
    bounce like the others and stays one k_bounce launch."""
    for k, v in knobs.items():
        monkeypatch.setenv(k, v)
    c = S.case(name, oracle)
    mode = S.CASES[name][-1]
    g = S.gpu_scene(P, c, mode)
    depth = 4
    want, _ = S.restated(c, depth, mode)
    sums = S.pass_order_sums(want, W, H, SPP)
    _, st = _raw(torch, g, P.render_params(W, H, SPP, depth, passes_per_batch=1, time_kernels=True))
    assert st["kernel_launches"]["generate"] == 3
    if two_kernels:
        assert st["kernel_launches"]["trace"] > 0 and st["kernel_launches"]["shade"] > 0 and st["kernel_launches"]["bounce"] == 0
    else:
        assert st["kernel_launches"]["trace"] == 0 and st["kernel_launches"]["bounce"] == 3 * depth
    buf = torch.zeros((H, W, 3), dtype=torch.float64, device="cuda:0")
    for _ in range(2):  # two frames queued one behind the other
        g.render_raw_device(P.render_params(W, H, SPP, depth, passes_per_batch=1, asynchronous=True), buf.data_ptr())
    torch.cuda.synchronize()
    assert np.array_equal(bits(buf.cpu().numpy()), bits(sums))
    g.close()


@pytest.mark.parametrize("band_first", [0, 1])
def test_bands_are_the_rows_of_the_frame(P, oracle, torch, band_first):
    w, h, depth = 13, 19, 4  # bands of 8 rows dealt to 2 ranks: rank 0 rows 0-7 and 16-18, rank 1 rows 8-15
    c = S.case("shirley", oracle, w, h)
    g = S.gpu_scene(P, c)
    whole, _ = _raw(torch, g, P.render_params(w, h, SPP, depth, passes_per_batch=1))
    want, _ = S.restated(c, depth, 0, width=w, height=h)
    assert np.array_equal(bits(whole), bits(S.pass_order_sums(want, w, h, SPP)))
    params = P.render_params(w, h, SPP, depth, passes_per_batch=1, band_rows=8, band_first=band_first, band_step=2)
    rows = P.lib().ptx_local_rows(C.byref(params))
    assert rows == (11 if band_first == 0 else 8)
    band, _ = _raw(torch, g, params, rows)
    global_rows = [P.lib().ptx_global_row(C.byref(params), k) for k in range(rows)]
    assert np.array_equal(bits(band), bits(whole[global_rows]))
    g.close()


# ------------------------------------------------------------------------------------------------ the route is the only difference
def test_lens_on_then_off_is_a_scene_never_touched(P, oracle, torch):
    w, h, spp, depth = 64, 32, 4, 8
    c = S.case("shirley", oracle, w, h)
    fresh, touched = S.gpu_scene(P, c, lens=False), S.gpu_scene(P, c, lens=False)
    touched.set_lens(*c["lens"])
    on, _ = _raw(torch, touched, P.render_params(w, h, spp, depth))
    touched.set_lens(0.0, c["lens"][1])
    assert touched.lens() == (0.0, c["lens"][1])
    for kw in ({}, {"count_work": True}):
        a, sa = _raw(torch, fresh, P.render_params(w, h, spp, depth, **kw))
        b, sb = _raw(torch, touched, P.render_params(w, h, spp, depth, **kw))
        assert np.array_equal(bits(a), bits(b)) and not np.array_equal(bits(a), bits(on))
        for key in ("carry_launches", "primary_lane_walks", "lds_oct_launches", "segments"):
            assert sa[key] == sb[key], key
    assert sa["carry_launches"] > 0  # the pinhole's Shirley does take the shade-first order: the lens render above did not
    a, _ = fresh.render(w, h, spp, depth)
    b, _ = touched.render(w, h, spp, depth)
    assert np.array_equal(bits(a), bits(b))
    assert fresh.tile_list_stats() == touched.tile_list_stats()
    fresh.close()
    touched.close()


def test_the_setter_is_refused_while_a_render_runs(P, oracle):
    c = S.case("shirley", oracle, 64, 32)
    g = S.gpu_scene(P, c)
    seen = []

    def progress(n):
        seen.append(P.lib().ptx_scene_set_lens(g._h, 0.0, 1.0))
    g.render(64, 32, 2, 4, progress=progress)
    assert seen and set(seen) == {-3}  # PTX_ERR_STATE
    assert "while a render runs" in P.last_error()
    assert g.lens() == c["lens"]
    g.close()


# ------------------------------------------------------------------------------------------------ the drivers
@pytest.fixture(scope="module")
def frame(P, oracle):
    depth, n = 4, 6
    c = S.case("shirley", oracle)
    g = S.gpu_scene(P, c)
    rgb, _ = g.render(W, H, n, depth, passes_per_batch=2)
    yield c, g, n, depth, rgb.copy()
    g.close()


def test_the_frame_is_the_film_of_the_restated_sums(P, oracle, torch, frame):
    c, g, n, depth, rgb = frame
    xs, ys, ps = S.all_samples(W, H, n)
    want, _ = S.restated(c, depth, 0, spp=n, samples=(xs, ys, ps))
    sums = torch.tensor(S.pass_order_sums(want, W, H, n), device="cuda:0")
    out = torch.zeros_like(sums)
    P.film_resolve_device(0, W, H, n, sums.data_ptr(), out.data_ptr())
    assert np.array_equal(bits(out.cpu().numpy()), bits(rgb))


def test_progressive_denoised_and_adaptive_run_to_the_end_are_the_frame(P, frame):
    _, g, n, depth, rgb = frame
    got, _, done, _ = g.render_progressive(W, H, n, depth, passes_per_update=4)
    assert done == n and np.array_equal(bits(got), bits(rgb))
    got, _, _, done, _ = g.render_denoised(W, H, n, depth, passes_per_update=4, denoise={"levels": 0})
    assert done == n and np.array_equal(bits(got), bits(rgb))
    got, _, passes, _ = g.render_adaptive(W, H, n, depth, 0.0, min_passes=2, passes_per_round=3)
    assert (passes == n).all() and np.array_equal(bits(got), bits(rgb))


def test_a_pixel_list_gives_those_pixels_of_the_frame(P, torch, frame):
    _, g, n, depth, _ = frame
    params = P.render_params(W, H, n, depth, passes_per_batch=4)
    whole, _ = _raw(torch, g, params)
    pix = np.random.default_rng(9).choice(W * H, 37, replace=False).astype(np.int32)  # ragged: no multiple of a wave, unordered
    d_pix = torch.tensor(pix, device="cuda:0")
    raw = torch.zeros((H, W, 3), dtype=torch.float64, device="cuda:0")
    st = g.render_pixels_device(params, 0, n, d_pix.data_ptr(), len(pix), raw.data_ptr())
    raw = raw.cpu().numpy().reshape(-1, 3)
    assert st["samples"] == len(pix) * n
    assert np.array_equal(bits(raw[pix]), bits(whole.reshape(-1, 3)[pix]))
    rest = np.setdiff1d(np.arange(W * H), pix)
    assert (raw[rest] == 0.0).all()


def test_replicas_carry_the_lens(P, frame, monkeypatch):
    c, g, n, depth, rgb = frame
    monkeypatch.setenv("PTX_MULTI_ALIAS", "1")  # test hook: replicas may share a device
    r = g.replicate(0)
    assert r.lens() == g.lens() == c["lens"]
    got, _ = P.render_multi([g, r], W, H, n, depth)
    assert np.array_equal(bits(got), bits(rgb))
    # a replica with another lens is not a replica of the same picture
    r.set_lens(c["lens"][0] * 2.0, c["lens"][1])
    with pytest.raises(P.PtxError, match="does not carry the lens"):
        P.render_multi([g, r], W, H, n, depth)
    r.close()
    # the replicas a scene owns follow the setter
    got, _ = g.render(W, H, n, depth, n_gpus=2)
    assert np.array_equal(bits(got), bits(rgb))
    g.set_lens(c["lens"][0] * 2.0, c["lens"][1])
    one, _ = g.render(W, H, n, depth)
    two, _ = g.render(W, H, n, depth, n_gpus=2)
    g.set_lens(*c["lens"])
    assert np.array_equal(bits(one), bits(two)) and not np.array_equal(bits(one), bits(rgb))


@pytest.mark.parametrize("name", ["shirley", "mesh", "image"])
def test_features_are_the_first_hit_of_the_lens_ray(P, oracle, torch, name):
    """hits, depth (t along the lens ray), albedo and the facing normal of every sample, summed per pixel in pass order"""
    c = S.case(name, oracle)
    g = S.gpu_scene(P, c)
    depth = 4
    feat = torch.zeros((H, W, 8), dtype=torch.float64, device="cuda:0")
    params = P.render_params(W, H, SPP, depth, passes_per_batch=2)
    g.render_features_device(params, 0, 2, feat.data_ptr())
    g.render_features_device(params, 2, 1, feat.data_ptr())
    xs, ys, ps = S.all_samples()
    want = c["ref"].first_hits(c["lens"], W, H, SPP, depth, xs, ys, ps, c["images"], c["env"]).reshape(H * W, SPP, 8)
    sums = np.zeros((H * W, 8))
    for k in range(SPP):
        sums = sums + want[:, k]
    got = feat.cpu().numpy().reshape(-1, 8)
    assert np.array_equal(got[:, 7], sums[:, 7]) and 0 < sums[:, 7].sum()
    assert np.array_equal(bits(got[:, 6]), bits(sums[:, 6])), "depth"
    assert np.array_equal(bits(got[:, :3]), bits(sums[:, :3])), "albedo"
    assert np.array_equal(bits(got[:, 3:6]), bits(sums[:, 3:6])), "normal"
    pin = c["ref"].first_hits((0.0, 1.0), W, H, SPP, depth, xs, ys, ps, c["images"], c["env"])
    assert not np.array_equal(bits(pin[:, 6]), bits(want.reshape(-1, 8)[:, 6]))
    g.close()


# ------------------------------------------------------------------------------------------------ refusals
def test_the_pinhole_only_entry_points_refuse_a_lens(P, oracle):
    c = S.case("cornell", oracle, 16, 8)
    g = S.gpu_scene(P, c)
    xs, ys, ps = (np.zeros(4, dtype=np.int32) for _ in range(3))
    p = P.render_params(16, 8, 1, 4)
    ray, attn, alive = np.zeros((4, 6)), np.zeros((4, 3)), np.zeros(4, dtype=np.int32)
    P.lib().ptx_debug_first_scatter.argtypes = [C.c_void_p, C.POINTER(P.abi.RenderParams), C.c_int64, S.ip, S.ip, S.ip, S.dp, S.dp, S.ip]
    args = (g._h, C.byref(p), 4, S._ip(xs), S._ip(ys), S._ip(ps), S._dp(ray), S._dp(attn), S._ip(alive))
    assert P.lib().ptx_debug_first_scatter(*args) == -3
    assert "ptx_scene_set_lens" in P.last_error()
    lights = oracle.lights_cornell(16, 8)
    with pytest.raises(P.PtxError, match="ptx_scene_set_lens"):
        g.ppm_render(P.abi.ppm_params(16, 8, iterations=1, photon_count=2000), lights)
    g.set_lens(0.0, 1.0)  # off: both run
    assert P.lib().ptx_debug_first_scatter(*args) == 0, P.last_error()
    g.ppm_render(P.abi.ppm_params(16, 8, iterations=1, photon_count=2000), lights)
    g.close()


# ------------------------------------------------------------------------------------------------ CLI
def test_cli_lens_flags(P, tmp_path):
    """shirley_spheres --lens-radius=R [--focus-distance=F] writes the PNG the same calls give through Python; without
    --focus-distance the lens focuses on the camera's look-at target"""
    import os
    import subprocess
    from path_tracer_ocaml_amd import host
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    w, h, spp = 96, 48, 4
    hs = host.shirley_spheres(w, h)
    assert abs(hs.focus_distance - (13.0 ** 2 + 2.0 ** 2 + 4.5 ** 2) ** 0.5) < 1e-12
    g = P.Scene(hs.ptr, 0, keepalive=hs)
    plain, _ = g.render(w, h, spp, 8)
    for flags, lens in ((["--lens-radius=0.25"], (0.25, hs.focus_distance)), (["--lens-radius=0.25", "--focus-distance=9.5"], (0.25, 9.5))):
        g.set_lens(*lens)
        want, _ = g.render(w, h, spp, 8)
        assert not np.array_equal(bits(want), bits(plain))
        host.write_png(str(tmp_path / "want.png"), want)
        out = tmp_path / "got.png"
        r = subprocess.run([os.path.join(root, "path_tracer_ocaml_amd", "shirley_spheres"), f"--dimension={w},{h}", f"--samples-per-pixel={spp}",
                            "--no-progress", *flags, "-o", str(out)], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        assert out.read_bytes() == (tmp_path / "want.png").read_bytes(), flags
    g.close()
