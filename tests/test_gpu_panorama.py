"""The lat-long projection on the GPU (include/ptx.h, ptx_scene_set_camera_projection).

* ptx_camera_rays of a LATLONG scene is the numpy rule (tests/projection_reference.py) bit for bit at 1 x 1, 8 x 8, 9 x 7 and
  33 x 17, with no pose, under the identity pose and under an oblique one;
* a panorama's samples (ptx_trace_samples) are what ptx_render_rays gives for those rays at those offsets, bit for bit, with the same
  segment and work counters: the two new parts check each other;
* on the six scenes of the lens tests at 13 x 11: the raw sums are the pass-order fold of the per-sample values; the progressive
  render run to the end and the adaptive render at T = 0 are the frame; a ragged pixel list gives those pixels' sums; the features
  are the restatement's first hits of the panorama's rays;
* ptx_render_temporal, ptx_ppm_render and ptx_debug_first_scatter refuse a LATLONG scene; ptx_scene_replicate copies the projection
  and ptx_render_multi wants it equal on every scene.

Without the feature there is no such projection: every test here fails.
"""
import ctypes as C

import numpy as np
import pytest

import camera_pose_support as CS
import projection_reference as PR
import rays_support as RS
from rays_support import bits

pytestmark = pytest.mark.gpu
W, H, SPP = RS.W, RS.H, RS.SPP
PTX_ERR_STATE = -3
WAY_OUT = "ptx_scene_set_camera_projection(scene, PTX_PROJECTION_PERSPECTIVE) first"


@pytest.fixture(scope="module")
def P():
    import path_tracer_ocaml_amd as P
    assert P.lib().ptx_device_count() >= 1, P.last_error()
    return P


@pytest.fixture(scope="module")
def torch():
    return pytest.importorskip("torch")


def pano_scene(P, c, pose=None, mode=0):
    g = CS.gpu_scene(P, c, pose, mode, lens=False)
    g.set_camera_projection("latlong")
    return g


# ------------------------------------------------------------------------------------------------ the rays
@pytest.mark.parametrize("pose", ["none", "identity", "oblique"])
def test_camera_rays_equal_the_numpy_rule(P, oracle, pose):
    depth, spp = 4, 3
    c = RS.case("shirley", oracle)
    ps = {"none": None, "identity": CS.Pose(CS.ZERO, CS.IDENTITY), "oblique": c["poses"]["oblique"]}[pose]
    g = pano_scene(P, c, ps)
    for w, h in ((1, 1), (8, 8), (9, 7), (33, 17)):
        xs, ys, passes = RS.all_samples(w, h, spp)
        o, d = g.camera_rays(w, h, spp, depth, xs, ys, passes)
        cxcy, _ = PR.film_coordinates(w, h, spp, 2 + 2 * depth, xs, ys, passes)
        wo, wd = PR.latlong_rays(CS.ZERO if ps is None else ps.origin, CS.IDENTITY if ps is None else ps.rotation, cxcy)
        assert np.array_equal(bits(o), bits(wo)) and np.array_equal(bits(d), bits(wd)), (w, h)
    # back to the pinhole: the scene's own (or the pose's) rays again
    g.set_camera_projection("perspective")
    xs, ys, passes = RS.all_samples(9, 7, spp)
    o, d = g.camera_rays(9, 7, spp, depth, xs, ys, passes)
    home = c["ref"].rays(ps, 9, 7, spp, depth, xs, ys, passes)
    assert np.array_equal(bits(d), bits(home[:, 3:]))
    g.close()


# ------------------------------------------------------------------------------------------------ per sample: the two parts meet
@pytest.mark.parametrize("name", list(RS.CASES))
def test_a_panoramas_samples_are_render_rays_on_its_camera_rays(P, oracle, name):
    c = RS.case(name, oracle)
    mode = RS.CASES[name][-1]
    xs, ys, ps = RS.all_samples()
    offsets = RS.frame_offsets()
    for pose in (None, c["poses"]["oblique"]):
        g = pano_scene(P, c, pose, mode)
        seen = 0.0
        for depth in RS.DEPTHS:
            o, d = g.camera_rays(W, H, SPP, depth, xs, ys, ps)
            want, wst = g.trace_samples(W, H, SPP, depth, xs, ys, ps, count_work=True)
            got, _, st = g.render_rays(o, d, offsets, max_bounces=depth, count_work=True)
            nbad = int((bits(got) != bits(want)).any(axis=1).sum())
            assert nbad == 0, f"{name} depth {depth}: {nbad} of {len(xs)} samples differ"
            keys = ("samples", "segments", "nodes_tested", "prims_tested", "floor_tested")
            print(name, depth, {k: (st[k], wst[k]) for k in keys})
            assert [st[k] for k in keys] == [wst[k] for k in keys]
            assert wst["carry_launches"] == 0 and wst["solo_launches"] == 0
            # ... and the restatement's path loop on those rays
            ref, segments = c["rays_ref"].trace_rays(np.concatenate([o, d], axis=1), offsets, depth, None, c["images"], c["env"], mode,
                                                     c["sampling"])
            assert np.array_equal(bits(0.0 + want), bits(0.0 + ref)) and wst["segments"] == segments
            seen = max(seen, float(want.max()))
        assert seen > 0.0
        g.close()


# ------------------------------------------------------------------------------------------------ the drivers
@pytest.fixture(scope="module", params=list(RS.CASES))
def frame(request, P, oracle):
    """a 13 x 11 panorama of a case from its oblique pose: the scene, its per-sample values at depth 4 and its rays"""
    name = request.param
    c = RS.case(name, oracle)
    g = pano_scene(P, c, c["poses"]["oblique"], RS.CASES[name][-1])
    xs, ys, ps = RS.all_samples()
    samples, _ = g.trace_samples(W, H, SPP, 4, xs, ys, ps)
    rgb, _ = g.render(W, H, SPP, 4, passes_per_batch=2)
    yield name, c, g, samples, rgb.copy()
    g.close()


def test_raw_sums_are_the_samples_in_pass_order(P, torch, frame):
    name, c, g, samples, _ = frame
    want = RS.LS.pass_order_sums(samples, W, H, SPP)
    for ppb in (1, 2, 0):
        buf = torch.zeros((H, W, 3), dtype=torch.float64, device="cuda:0")
        st = g.render_raw_device(P.render_params(W, H, SPP, 4, passes_per_batch=ppb, count_work=True), buf.data_ptr())
        assert np.array_equal(bits(buf.cpu().numpy()), bits(want)), (name, ppb)
        assert st["carry_launches"] == 0 and st["solo_launches"] == 0 and st["lds_oct_launches"] == 0
    # slices of passes onto the same buffer
    buf = torch.zeros((H, W, 3), dtype=torch.float64, device="cuda:0")
    params = P.render_params(W, H, SPP, 4)
    g.render_passes_device(params, 0, 2, buf.data_ptr())
    g.render_passes_device(params, 2, 1, buf.data_ptr())
    assert np.array_equal(bits(buf.cpu().numpy()), bits(want)), name


def test_the_frame_is_the_film_of_those_sums_and_every_driver_renders_it(P, torch, frame):
    name, c, g, samples, rgb = frame
    sums = torch.tensor(RS.LS.pass_order_sums(samples, W, H, SPP), device="cuda:0")
    out = torch.zeros_like(sums)
    P.film_resolve_device(0, W, H, SPP, sums.data_ptr(), out.data_ptr())
    assert np.array_equal(bits(out.cpu().numpy()), bits(rgb)), name
    got, _, done, _ = g.render_progressive(W, H, SPP, 4, passes_per_update=2)
    assert done == SPP and np.array_equal(bits(got), bits(rgb)), name
    got, _, passes, _ = g.render_adaptive(W, H, SPP, 4, 0.0, min_passes=2, passes_per_round=1)
    assert (passes == SPP).all() and np.array_equal(bits(got), bits(rgb)), name
    got, _, _, done, _ = g.render_denoised(W, H, SPP, 4, passes_per_update=2, denoise={"levels": 0})
    assert done == SPP and np.array_equal(bits(got), bits(rgb)), name


def test_a_ragged_pixel_list_gives_those_pixels_sums(P, torch, frame):
    name, c, g, samples, _ = frame
    want = RS.LS.pass_order_sums(samples, W, H, SPP).reshape(-1, 3)
    pix = np.random.default_rng(9).choice(W * H, 37, replace=False).astype(np.int32)  # no multiple of a wave, unordered
    d_pix = torch.tensor(pix, device="cuda:0")
    raw = torch.zeros((H, W, 3), dtype=torch.float64, device="cuda:0")
    st = g.render_pixels_device(P.render_params(W, H, SPP, 4, passes_per_batch=2), 0, SPP, d_pix.data_ptr(), len(pix), raw.data_ptr())
    raw = raw.cpu().numpy().reshape(-1, 3)
    assert st["samples"] == len(pix) * SPP
    assert np.array_equal(bits(raw[pix]), bits(want[pix])), name
    assert (raw[np.setdiff1d(np.arange(W * H), pix)] == 0.0).all()


def test_features_are_the_first_hits_of_the_panoramas_rays(P, torch, frame):
    name, c, g, _, _ = frame
    xs, ys, ps = RS.all_samples()
    o, d = g.camera_rays(W, H, SPP, 4, xs, ys, ps)
    want = c["rays_ref"].first_hits(np.concatenate([o, d], axis=1), c["images"], c["env"]).reshape(H * W, SPP, 8)
    sums = np.zeros((H * W, 8))
    for k in range(SPP):
        sums = sums + want[:, k]
    feat = torch.zeros((H, W, 8), dtype=torch.float64, device="cuda:0")
    params = P.render_params(W, H, SPP, 4, passes_per_batch=2)
    g.render_features_device(params, 0, 2, feat.data_ptr())
    g.render_features_device(params, 2, 1, feat.data_ptr())
    got = feat.cpu().numpy().reshape(-1, 8)
    assert np.array_equal(got[:, 7], sums[:, 7]) and 0 < sums[:, 7].sum(), name
    assert np.array_equal(bits(got[:, 6]), bits(sums[:, 6])), "depth"
    assert np.array_equal(bits(got[:, :3]), bits(sums[:, :3])), "albedo"
    assert np.array_equal(bits(got[:, 3:6]), bits(sums[:, 3:6])), "normal"


# ------------------------------------------------------------------------------------------------ refusals, replicas
def test_the_pinhole_only_entry_points_refuse_a_panorama(P, oracle):
    c = RS.case("cornell", oracle)
    g = pano_scene(P, c)
    with pytest.raises(P.PtxError) as e:
        g.render_temporal(W, H, 4, 4, 0, 4)
    assert "(-3)" in str(e.value) and WAY_OUT in str(e.value)
    with pytest.raises(P.PtxError) as e:
        g.ppm_render(P.abi.ppm_params(W, H, iterations=1, photon_count=2000), oracle.lights_cornell(W, H))
    assert "(-3)" in str(e.value) and WAY_OUT in str(e.value)
    L = P.lib()
    ip, dp = P.abi.c_int32_p, P.abi.c_double_p
    xs = np.zeros(4, dtype=np.int32)
    p = P.render_params(W, H, 4, 4)
    ray, attn, alive = np.zeros((4, 6)), np.zeros((4, 3)), np.zeros(4, dtype=np.int32)
    L.ptx_debug_first_scatter.argtypes = [C.c_void_p, C.POINTER(P.abi.RenderParams), C.c_int64, ip, ip, ip, dp, dp, ip]
    rc = L.ptx_debug_first_scatter(g._h, C.byref(p), 4, xs.ctypes.data_as(ip), xs.ctypes.data_as(ip), xs.ctypes.data_as(ip),
                                   ray.ctypes.data_as(dp), attn.ctypes.data_as(dp), alive.ctypes.data_as(ip))
    assert rc == PTX_ERR_STATE and WAY_OUT in P.last_error()
    assert not ray.any() and not alive.any()
    # the setter is refused while a render runs
    seen = []
    g.render(64, 32, 2, 4, progress=lambda n: seen.append(L.ptx_scene_set_camera_projection(g._h, 0)))
    assert seen and set(seen) == {PTX_ERR_STATE} and g.camera_projection == "latlong"
    g.close()


def test_replicas_carry_the_projection(P, oracle, monkeypatch):
    c = RS.case("shirley", oracle)
    g = pano_scene(P, c, c["poses"]["oblique"])
    rgb, _ = g.render(W, H, SPP, 4)
    monkeypatch.setenv("PTX_MULTI_ALIAS", "1")  # test hook: replicas may share a device
    r = g.replicate(0)
    assert r.camera_projection == "latlong"
    got, _ = P.render_multi([g, r], W, H, SPP, 4)
    assert np.array_equal(bits(got), bits(rgb))
    r.set_camera_projection("perspective")
    with pytest.raises(P.PtxError, match="does not carry the camera projection"):
        P.render_multi([g, r], W, H, SPP, 4)
    r.close()
    got, _ = g.render(W, H, SPP, 4, n_gpus=2)  # the replicas a scene owns follow the setter
    assert np.array_equal(bits(got), bits(rgb))
    g.set_camera_projection("perspective")
    pin, _ = g.render(W, H, SPP, 4, n_gpus=2)
    assert not np.array_equal(bits(pin), bits(rgb))
    g.close()
