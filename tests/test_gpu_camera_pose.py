"""The camera pose on the GPU (include/ptx.h, ptx_scene_set_camera_pose) against the restatement tests/c/camera_pose_oracle.c.

* ptx_camera_rays is the restatement's ray bit for bit, at frame sizes from one pixel to ragged and many-tile ones, with and without
  a lens and a view override;
* per-sample radiance (ptx_trace_samples) at depths 0, 1 and 8 is the restatement's bit for bit on the six scenes of the lens tests,
  from an oblique pose, from INSIDE the large glass sphere, from below the ground's surface and through a view override;
* the identity pose at origin 0 renders the pinhole's raw sums bit for bit -- and, with a lens, the lens render's -- through another
  route: generated rays, the walk-first order, no tile lists.  Without the feature there is no such call: this test fails;
* every driver (raw sums, bands, many batches, progressive, adaptive, denoised, a pixel list, features, replicas) gives the
  per-sample values; a posed scene never takes the shade-first order, the per-octant image or a solo run, and with the pose off again
  it schedules what it scheduled before.

tests/test_camera_pose_reference.py asserts that the restatement's posed rays differ from the scene's own on every sample.
"""
import ctypes as C

import numpy as np
import pytest

import camera_pose_support as S

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


# ------------------------------------------------------------------------------------------------ the rays
@pytest.mark.parametrize("lens", [False, True])
@pytest.mark.parametrize("pose", ["oblique", "view", "below_ground"])
def test_camera_rays_equal_the_restatement(P, oracle, pose, lens):
    depth, spp = 4, 4
    c = S.case("shirley", oracle)  # (the film coordinates depend on the frame's size, the view on the descriptor alone)
    ps = c["poses"][pose]
    for w, h in ((1, 1), (8, 8), (13, 7), (257, 1), (64, 8)):
        g = S.gpu_scene(P, c, ps, lens=lens)
        xs, ys, passes = S.all_samples(w, h, spp)  # passes 0 .. 3
        o, d = g.camera_rays(w, h, spp, depth, xs, ys, passes)
        want = c["ref"].rays(ps, w, h, spp, depth, xs, ys, passes, c["lens"] if lens else None)
        assert np.array_equal(bits(o), bits(want[:, :3])) and np.array_equal(bits(d), bits(want[:, 3:])), (w, h)
        if (w, h) == (13, 7):  # with the pose off: the scene's own rays, through the existing generators
            g.set_camera_pose()
            o, d = g.camera_rays(w, h, spp, depth, xs, ys, passes)
            home = c["ref"].rays(None, w, h, spp, depth, xs, ys, passes, c["lens"] if lens else None)
            assert np.array_equal(bits(np.concatenate([o, d], axis=1)), bits(home))
            assert (bits(home) != bits(want)).any(axis=1).all()
        g.close()


# ------------------------------------------------------------------------------------------------ per sample
@pytest.mark.parametrize("name", list(S.CASES))
def test_samples_equal_the_restatement(P, oracle, name):
    c = S.case(name, oracle)
    mode = S.CASES[name][-1]
    assert {"oblique", "view"} <= set(c["poses"])
    if name.startswith("shirley") or name in ("image", "envlight"):
        assert {"inside_glass", "below_ground"} <= set(c["poses"])
    xs, ys, ps = S.all_samples()
    g = S.gpu_scene(P, c, None, mode)
    for pose_name, pose in c["poses"].items():
        pose.set_on(g)
        for depth in S.DEPTHS:
            got, st = g.trace_samples(W, H, SPP, depth, xs, ys, ps, count_work=True)
            want, segments = S.restated(c, pose, depth, mode)
            nbad = int((bits(got) != bits(want)).any(axis=1).sum())
            assert nbad == 0, f"{name} {pose_name} mode {mode} depth {depth}: {nbad} of {len(xs)} samples differ"
            assert st["segments"] == segments and st["carry_launches"] == 0 and st["solo_launches"] == 0
            if c["lds"] is not None:
                assert st["traversal_in_lds"] == bool(c["lds"]), name
        assert float(want.max()) > 0.0, pose_name
    g.close()


def test_samples_under_a_pose_and_a_lens(P, oracle):
    c = S.case("shirley", oracle)
    xs, ys, ps = S.all_samples()
    pose = c["poses"]["inside_glass"]
    g = S.gpu_scene(P, c, pose, lens=True)
    for depth in S.DEPTHS:
        got, _ = g.trace_samples(W, H, SPP, depth, xs, ys, ps)
        want, _ = S.restated(c, pose, depth, lens=True)
        assert np.array_equal(bits(got), bits(want)), depth
    assert not np.array_equal(bits(want), bits(S.restated(c, pose, 8)[0]))  # the lens is not ignored
    g.close()


# ------------------------------------------------------------------------------------------------ identity pose == the scene's own camera
@pytest.mark.parametrize("name, w, h, spp, depth", [("shirley", 13, 7, 4, 4), ("shirley", 64, 40, 4, 4), ("cornell", 16, 16, 4, 8)])
@pytest.mark.parametrize("lens", [False, True])
def test_the_identity_pose_renders_the_pinholes_sums(P, oracle, torch, name, w, h, spp, depth, lens):
    """order, ids, holes and offsets of the generator against the fused camera launch's (or the lens kind of k_generate_tiles), and
    the counters of a posed render; with the pose off again the scene reports what it reported before"""
    c = S.case(name, oracle, w, h)
    g = S.gpu_scene(P, c, None, lens=lens)
    params, counting = P.render_params(w, h, spp, depth), P.render_params(w, h, spp, depth, count_work=True)
    home, _ = _raw(torch, g, params)
    _, before = _raw(torch, g, counting)
    lists_before = g.tile_list_stats()
    g.set_camera_pose(np.zeros(3), np.eye(3))
    posed, _ = _raw(torch, g, params)
    assert np.array_equal(bits(posed), bits(home)) and float(home.max()) > 0.0
    counted, st = _raw(torch, g, counting)
    assert np.array_equal(bits(counted), bits(home))
    assert st["carry_launches"] == 0 and st["lds_oct_launches"] == 0 and st["solo_launches"] == 0 and st["primary_lane_walks"] == 0
    assert st["segments"] == before["segments"]
    timed, st = _raw(torch, g, P.render_params(w, h, spp, depth, time_kernels=True))
    assert st["kernel_launches"]["generate"] >= 1 and np.array_equal(bits(timed), bits(home))
    assert g.tile_list_stats() == lists_before  # a posed render builds and scans no tile lists
    g.set_camera_pose()
    again, _ = _raw(torch, g, params)
    _, after = _raw(torch, g, counting)
    assert np.array_equal(bits(again), bits(home))
    for key in ("carry_launches", "lds_oct_launches", "solo_launches", "primary_lane_walks", "segments"):
        assert after[key] == before[key], key
    if name == "shirley" and not lens:
        assert before["carry_launches"] > 0  # the scene's own camera does take the shade-first order
    g.close()


# ------------------------------------------------------------------------------------------------ the drivers
@pytest.mark.parametrize("name, pose", [("shirley", "oblique"), ("shirley", "inside_glass"), ("cornell", "view"), ("mesh", "oblique")])
def test_raw_sums_are_the_samples_in_pass_order(P, oracle, torch, name, pose):
    """passes_per_batch = 1: three batches, both streams"""
    c = S.case(name, oracle)
    mode = S.CASES[name][-1]
    ps = c["poses"][pose]
    g = S.gpu_scene(P, c, ps, mode)
    depth = 4
    raw, _ = _raw(torch, g, P.render_params(W, H, SPP, depth, passes_per_batch=1))
    want, segments = S.restated(c, ps, depth, mode)
    assert np.array_equal(bits(raw), bits(S.pass_order_sums(want, W, H, SPP)))
    _, st = _raw(torch, g, P.render_params(W, H, SPP, depth, passes_per_batch=1, count_work=True))
    assert st["segments"] == segments and st["carry_launches"] == 0 and st["lds_oct_launches"] == 0 and st["solo_launches"] == 0
    timed, st = _raw(torch, g, P.render_params(W, H, SPP, depth, passes_per_batch=1, time_kernels=True))
    assert st["kernel_launches"]["generate"] == 3 and np.array_equal(bits(timed), bits(raw))
    assert g.tile_list_stats()["list_launches"] == 0
    buf = torch.zeros((H, W, 3), dtype=torch.float64, device="cuda:0")
    g.render_raw_device(P.render_params(W, H, SPP, depth, passes_per_batch=1, asynchronous=True), buf.data_ptr())
    torch.cuda.synchronize()
    assert np.array_equal(bits(buf.cpu().numpy()), bits(raw))
    g.close()


def test_batches_forced_by_PTX_BATCH_PATHS(P, oracle, torch, monkeypatch):
    """PTX_BATCH_PATHS has a floor of 2^20 paths a batch, so the frame is large enough to be cut: 640 x 480, 8 passes = 2.4 M paths
    -> three batches by size, made four so that both streams get as many.  Too many samples to restate on the CPU in a test: a
    random 1500 pixels are compared with their per-sample values (ptx_trace_samples, which the tests above tie to the restatement)
    and the whole frame with the same frame rendered in ONE batch."""
    w, h, spp, depth = 640, 480, 8, 4
    c = S.case("shirley", oracle, w, h)
    pose = c["poses"]["oblique"]
    g = S.gpu_scene(P, c, pose)
    one, st = _raw(torch, g, P.render_params(w, h, spp, depth, passes_per_batch=spp, time_kernels=True))
    assert st["kernel_launches"]["generate"] == 1
    monkeypatch.setenv("PTX_BATCH_PATHS", "1")
    many, st = _raw(torch, g, P.render_params(w, h, spp, depth, time_kernels=True))
    assert st["kernel_launches"]["generate"] == 4
    assert np.array_equal(bits(many), bits(one))
    pix = np.random.default_rng(4).choice(w * h, 1500, replace=False)
    xs, ys, ps = (np.repeat(pix % w, spp), np.repeat(pix // w, spp), np.tile(np.arange(spp), len(pix)))
    samples, _ = g.trace_samples(w, h, spp, depth, xs, ys, ps)
    sums = np.zeros((len(pix), 3))
    for k in range(spp):
        sums = sums + samples.reshape(len(pix), spp, 3)[:, k]
    assert np.array_equal(bits(many.reshape(-1, 3)[pix]), bits(sums))
    g.close()


@pytest.mark.parametrize("ranks", [2, 3])
def test_bands_are_the_rows_of_the_frame(P, oracle, torch, ranks):
    w, h, depth = 13, 27, 4  # bands of 8 rows dealt to the ranks; the last band is ragged
    c = S.case("shirley", oracle, w, h)
    pose = c["poses"]["oblique"]
    g = S.gpu_scene(P, c, pose)
    whole, _ = _raw(torch, g, P.render_params(w, h, SPP, depth, passes_per_batch=1))
    want, _ = S.restated(c, pose, depth, width=w, height=h)
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


@pytest.fixture(scope="module")
def frame(P, oracle):
    depth, n = 4, 6
    c = S.case("shirley", oracle)
    pose = c["poses"]["oblique"]
    g = S.gpu_scene(P, c, pose)
    rgb, _ = g.render(W, H, n, depth, passes_per_batch=2)
    yield c, pose, g, n, depth, rgb.copy()
    g.close()


def test_the_frame_is_the_film_of_the_restated_sums(P, torch, frame):
    c, pose, g, n, depth, rgb = frame
    xs, ys, ps = S.all_samples(W, H, n)
    want, _ = S.restated(c, pose, depth, spp=n, samples=(xs, ys, ps))
    sums = torch.tensor(S.pass_order_sums(want, W, H, n), device="cuda:0")
    out = torch.zeros_like(sums)
    P.film_resolve_device(0, W, H, n, sums.data_ptr(), out.data_ptr())
    assert np.array_equal(bits(out.cpu().numpy()), bits(rgb))


def test_progressive_denoised_and_adaptive_run_to_the_end_are_the_frame(P, frame):
    _, _, g, n, depth, rgb = frame
    got, _, done, _ = g.render_progressive(W, H, n, depth, passes_per_update=4)
    assert done == n and np.array_equal(bits(got), bits(rgb))
    got, _, _, done, _ = g.render_denoised(W, H, n, depth, passes_per_update=4, denoise={"levels": 0})
    assert done == n and np.array_equal(bits(got), bits(rgb))
    got, _, passes, _ = g.render_adaptive(W, H, n, depth, 0.0, min_passes=2, passes_per_round=3)
    assert (passes == n).all() and np.array_equal(bits(got), bits(rgb))


def test_a_pixel_list_gives_those_pixels_of_the_frame(P, torch, frame):
    _, _, g, n, depth, _ = frame
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


def test_replicas_carry_the_pose(P, frame, monkeypatch):
    c, pose, g, n, depth, rgb = frame
    monkeypatch.setenv("PTX_MULTI_ALIAS", "1")  # test hook: replicas may share a device
    r = g.replicate(0)
    ro, rR, rv = r.camera_pose
    go, gR, gv = g.camera_pose
    assert np.array_equal(ro, go) and np.array_equal(rR, gR) and rv == gv and np.array_equal(go, pose.origin)
    got, _ = P.render_multi([g, r], W, H, n, depth)
    assert np.array_equal(bits(got), bits(rgb))
    # a replica with another pose, or with none, is not a replica of the same picture
    r.set_camera_pose(pose.origin * 2.0, pose.rotation)
    with pytest.raises(P.PtxError, match="does not carry the camera pose"):
        P.render_multi([g, r], W, H, n, depth)
    r.set_camera_pose()
    with pytest.raises(P.PtxError, match="does not carry the camera pose"):
        P.render_multi([g, r], W, H, n, depth)
    r.close()
    # the replicas a scene owns follow the setter
    got, _ = g.render(W, H, n, depth, n_gpus=2)
    assert np.array_equal(bits(got), bits(rgb))
    c["poses"]["view"].set_on(g)
    one, _ = g.render(W, H, n, depth)
    two, _ = g.render(W, H, n, depth, n_gpus=2)
    pose.set_on(g)
    assert np.array_equal(bits(one), bits(two)) and not np.array_equal(bits(one), bits(rgb))


@pytest.mark.parametrize("name, pose", [("shirley", "inside_glass"), ("mesh", "oblique"), ("image", "below_ground")])
def test_features_are_the_first_hit_of_the_posed_ray(P, oracle, torch, name, pose):
    """hits, depth (t along the posed ray), albedo and the facing normal (scene space) of every sample, summed per pixel in pass order"""
    c = S.case(name, oracle)
    ps_ = c["poses"][pose]
    g = S.gpu_scene(P, c, ps_)
    depth = 4
    feat = torch.zeros((H, W, 8), dtype=torch.float64, device="cuda:0")
    params = P.render_params(W, H, SPP, depth, passes_per_batch=2)
    g.render_features_device(params, 0, 2, feat.data_ptr())
    g.render_features_device(params, 2, 1, feat.data_ptr())
    xs, ys, ps = S.all_samples()
    want = c["ref"].first_hits(ps_, W, H, SPP, depth, xs, ys, ps, c["images"], c["env"]).reshape(H * W, SPP, 8)
    sums = np.zeros((H * W, 8))
    for k in range(SPP):
        sums = sums + want[:, k]
    got = feat.cpu().numpy().reshape(-1, 8)
    assert np.array_equal(got[:, 7], sums[:, 7]) and 0 < sums[:, 7].sum()
    assert np.array_equal(bits(got[:, 6]), bits(sums[:, 6])), "depth"
    assert np.array_equal(bits(got[:, :3]), bits(sums[:, :3])), "albedo"
    assert np.array_equal(bits(got[:, 3:6]), bits(sums[:, 3:6])), "normal"
    g.close()


def test_a_pixel_list_and_the_features_under_a_pose_and_a_lens(P, oracle, torch):
    """pose + lens away from the explicit-sample list: the pixel-list generator and the rays-only tile generator that feeds the
    features, at a frame of two ragged tile columns and two ragged tile rows"""
    c = S.case("shirley", oracle)
    pose = c["poses"]["inside_glass"]
    g = S.gpu_scene(P, c, pose, lens=True)
    depth = 4
    params = P.render_params(W, H, SPP, depth)
    # the pixel list: those pixels of the raw sums, which are the restated samples in pass order
    want, _ = S.restated(c, pose, depth, lens=True)
    whole, _ = _raw(torch, g, params)
    assert np.array_equal(bits(whole), bits(S.pass_order_sums(want, W, H, SPP))) and float(want.max()) > 0.0
    assert not np.array_equal(bits(want), bits(S.restated(c, pose, depth)[0]))  # the lens is not ignored
    pix = np.random.default_rng(9).choice(W * H, 37, replace=False).astype(np.int32)  # ragged: no multiple of a wave, unordered
    d_pix = torch.tensor(pix, device="cuda:0")
    raw = torch.zeros((H, W, 3), dtype=torch.float64, device="cuda:0")
    st = g.render_pixels_device(params, 0, SPP, d_pix.data_ptr(), len(pix), raw.data_ptr())
    raw = raw.cpu().numpy().reshape(-1, 3)
    assert st["samples"] == len(pix) * SPP
    assert np.array_equal(bits(raw[pix]), bits(whole.reshape(-1, 3)[pix])) and float(raw[pix].max()) > 0.0
    rest = np.setdiff1d(np.arange(W * H), pix)
    assert (raw[rest] == 0.0).all()
    # the features, in two slices
    feat = torch.zeros((H, W, 8), dtype=torch.float64, device="cuda:0")
    sliced = P.render_params(W, H, SPP, depth, passes_per_batch=2)
    g.render_features_device(sliced, 0, 2, feat.data_ptr())
    g.render_features_device(sliced, 2, 1, feat.data_ptr())
    xs, ys, ps = S.all_samples()

    def sums_of(lens):
        hits = c["ref"].first_hits(pose, W, H, SPP, depth, xs, ys, ps, c["images"], c["env"], lens=lens).reshape(H * W, SPP, 8)
        sums = np.zeros((H * W, 8))
        for k in range(SPP):
            sums = sums + hits[:, k]
        return sums
    sums = sums_of(c["lens"])
    assert not np.array_equal(bits(sums), bits(sums_of(None)))  # the lens is not ignored
    got = feat.cpu().numpy().reshape(-1, 8)
    assert np.array_equal(got[:, 7], sums[:, 7]) and 0 < sums[:, 7].sum()
    assert np.array_equal(bits(got[:, 6]), bits(sums[:, 6])), "depth"
    assert np.array_equal(bits(got[:, :3]), bits(sums[:, :3])), "albedo"
    assert np.array_equal(bits(got[:, 3:6]), bits(sums[:, 3:6])), "normal"
    g.close()


def test_the_setter_is_refused_while_a_render_runs(P, oracle):
    c = S.case("shirley", oracle, 64, 32)
    pose = c["poses"]["oblique"]
    g = S.gpu_scene(P, c, pose)
    seen = []

    def progress(n):
        seen.append(P.lib().ptx_scene_set_camera_pose(g._h, None, None, None))
    g.render(64, 32, 2, 4, progress=progress)
    assert seen and set(seen) == {-3}  # PTX_ERR_STATE
    assert "while a render runs" in P.last_error()
    assert g.camera_pose is not None
    g.close()


# ------------------------------------------------------------------------------------------------ CLI
def _turntable_eye(cam, eye, target, frame, n):
    """render_command.cpp's pose_camera, operation for operation (the same libm)"""
    import math
    up = [float(u) for u in cam["up"]]
    ln = math.sqrt(up[0] * up[0] + up[1] * up[1] + up[2] * up[2])
    k = [u / ln for u in up]
    th = 2.0 * 3.14159265358979323846 * float(frame) / float(n)
    c, s = math.cos(th), math.sin(th)
    v = [eye[i] - target[i] for i in range(3)]
    kxv = [k[1] * v[2] - k[2] * v[1], k[2] * v[0] - k[0] * v[2], k[0] * v[1] - k[1] * v[0]]
    kv = k[0] * v[0] + k[1] * v[1] + k[2] * v[2]
    return [target[i] + (v[i] * c + kxv[i] * s + k[i] * kv * (1.0 - c)) for i in range(3)]


def test_cli_camera_flags(P, tmp_path):
    """shirley_spheres --camera-eye --camera-target [--camera-fov] writes the PNG the same calls give through Python, and --turntable=N
    writes N frames through one handle, each the PNG of its pose"""
    import os
    import subprocess
    from path_tracer_ocaml_amd import host
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = os.path.join(root, "path_tracer_ocaml_amd", "shirley_spheres")
    w, h, spp = 96, 48, 4
    hs = host.shirley_spheres(w, h)
    cam = hs.camera
    g = P.Scene(hs.ptr, 0, keepalive=hs)
    plain, _ = g.render(w, h, spp, 8)
    eye, target, fov = (9.0, 3.5, -6.0), (0.5, 0.4, 0.3), 28.0
    common = [exe, f"--dimension={w},{h}", f"--samples-per-pixel={spp}", "--no-progress"]

    def png_of(pose_eye, pose_target, pose_fov, name):
        g.set_camera_pose(*P.camera_pose_look_at(cam["look_at"], pose_eye, pose_target, cam["up"], w / h, pose_fov))
        want, _ = g.render(w, h, spp, 8)
        assert not np.array_equal(bits(want), bits(plain))
        host.write_png(str(tmp_path / name), want)
        return (tmp_path / name).read_bytes()
    for flags, f in ((["--camera-fov=28"], fov), ([], cam["fov_deg"])):
        out = tmp_path / "got.png"
        r = subprocess.run(common + ["--camera-eye=9,3.5,-6", "--camera-target=0.5,0.4,0.3", *flags, "-o", str(out)], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        assert out.read_bytes() == png_of(eye, target, f, "want.png"), flags
    n = 3
    r = subprocess.run(common + [f"--turntable={n}", "-o", str(tmp_path / "turn.png")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    own_eye, own_target = [float(v) for v in cam["eye"]], [float(v) for v in cam["target"]]
    frames = [(tmp_path / f"turn-{k:03d}.png").read_bytes() for k in range(n)]
    for k in range(n):
        assert frames[k] == png_of(_turntable_eye(cam, own_eye, own_target, k, n), own_target, cam["fov_deg"], f"want-{k}.png"), k
    assert len(set(frames)) == n and not (tmp_path / "turn.png").exists()
    g.close()
