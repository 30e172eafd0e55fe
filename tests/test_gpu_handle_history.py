"""One ptx_scene handle taken through many states, and pinned to the restatements in every one of them.

Every other GPU module creates a handle, sets the state its feature is about, renders and closes.  A host does the opposite: it keeps
one handle and changes it.  What such a handle caches -- the Schedule every setter must renew, queues whose record format follows
has_emit, hit buffers, one alpha table per sampler dimension, camera tile lists for up to eight image sizes, the slot categories and
shading records with images in place -- is revisited here: one test per walk of handle_history_support.WALKS, on ONE handle, and after
every step of it (a setter, a change of render parameters, a driver call, a call that is refused)

  the getters equal the model (a refused call returned the documented error and changed nothing);
  the plain check: ptx_render_features_device, then -- the launch record cleared -- ptx_render_raw_device and ptx_trace_samples over
    every sample of the frame equal the restatement of the model's state, bit for bit, on every sample, on the pass-order sums and on
    the first-hit feature sums, nothing excluded; counting runs report the reference's segments and, where the paths are the oracle's,
    its node, primitive and floor tests -- this render's, not a running total;
  the launched set equals test_gpu_kernel_coverage.expected() of the state at the step's depth: what a fresh handle would launch;
  after a refused call the check gives the bits of the check before it.

The features come first on purpose: ptx_render_features_device is the entry point that reads the handle's Schedule as the last setter
left it (the render drivers renew it from the batch plan), so it is the one a setter without its reschedule() shows in.

The restatements are CPU code and cached per (scene, state, depth, size): handle_history_support.reference."""
import math

import numpy as np
import pytest

import handle_history_support as HS
import test_gpu_kernel_coverage as KC

pytestmark = pytest.mark.gpu
SPP = HS.SPP


@pytest.fixture(scope="module")
def P():
    import path_tracer_ocaml_amd as P
    assert P.lib().ptx_device_count() >= 1, P.last_error()
    return P


@pytest.fixture(scope="module")
def torch():
    return pytest.importorskip("torch")


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _differ(a, b):
    a, b = _bits(a), _bits(b)
    assert a.shape == b.shape, (a.shape, b.shape)
    return int((a != b).any(axis=-1).sum())


def features_expected(case):
    """the one hot-family kernel a feature pass launches (features_queue, launch_trace in csrc/ptx_api.inc): k_trace on the camera rays,
    or -- behind a lens or a pose, whose rays are written into a queue first -- on queued rays that are no numbered bounce"""
    f, k = KC.SCENES[case.scene], {key[4:]: v for key, v in case.knobs}
    queued = case.lens or case.pose
    if f["lds"]:
        packet = not queued
    else:
        packet = k["OCT_IMAGE"] != 0 and not f.get("gap") and not k["TRACE_TOP"] != 0
    return "k_trace/%s/nocount/%s/%s/%s" % (f["mode"], "queued" if queued else "camera", "lds" if f["lds"] else "hbm",
                                            "packet" if packet else "nopacket")


class Handle:
    """the handle of a walk, the model's state beside it, and what the checks need to remember"""

    def __init__(self, P, torch, walk, monkeypatch):
        self.P, self.torch, self.walk, self.monkeypatch = P, torch, walk, monkeypatch
        for key, v in walk.knobs:
            monkeypatch.setenv(key, str(v))  # read when the handle is created
        ptr, keep = KC.scene(walk.scene)
        self.g = P.Scene(ptr, 0, keepalive=keep)
        self.grids = []      # the image sizes whose camera tile lists the handle keeps: the first eight it rendered with lists
        self.last = None     # the arrays of the check before

    def zeros(self, *shape, dtype=None):
        return self.torch.zeros(shape, dtype=dtype or self.torch.float64, device="cuda:0")

    # ---- the plain check
    def check(self, st, params, what):
        P, g, walk = self.P, self.g, self.walk
        w, h = HS.size_of(params.size)
        depth, count = params.depth, params.count
        ref = HS.reference(walk.scene, st, depth, params.size)
        case = HS.case_of(walk, st, params)
        xs, ys, ps = KC_samples(w, h)
        fig = {}
        if ref["features"] is not None:
            feat = self.zeros(h, w, 8)
            g.clear_launched_kernels()
            g.render_features_device(P.render_params(w, h, SPP, depth), 0, SPP, feat.data_ptr())
            fig["features_differ"] = _differ(feat.cpu().numpy().reshape(-1, 8), ref["features"])
            fig["features_launched"] = g.launched_kernels()
            assert fig["features_launched"] == [features_expected(case)], (what, fig["features_launched"])
        g.clear_launched_kernels()
        assert g.launched_kernels() == []
        raw = self.zeros(h, w, 3)
        st_r = g.render_raw_device(P.render_params(w, h, SPP, depth, count_work=count), raw.data_ptr())
        tiles = g.tile_list_stats()
        got, st_t = g.trace_samples(w, h, SPP, depth, xs, ys, ps, count_work=count)
        launched = g.launched_kernels()
        raw = raw.cpu().numpy()
        fig.update(samples_differ=_differ(got, ref["want"]), sums_differ=_differ(raw, ref["sums"]),
                   render={c: int(st_r[c]) for c in ("segments",) + KC.COUNTERS}, trace={c: int(st_t[c]) for c in ("segments",) + KC.COUNTERS},
                   tiles=tiles)
        want_launched = KC.expected(case, depth)
        # camera tile lists: a handle keeps those of the first eight sizes it rendered with lists; a further size walks
        lists_possible = any(name.endswith("/oct-tiles") for name in want_launched)
        if lists_possible and (w, h) not in self.grids and len(self.grids) < 8:
            self.grids.append((w, h))
        has_lists = lists_possible and (w, h) in self.grids
        if lists_possible and not has_lists:
            want_launched = {name[:-len("-tiles")] if name.endswith("/oct-tiles") else name for name in want_launched}
        print(what, fig, sorted(launched))
        assert fig["samples_differ"] == 0, what  # every sample of the frame, none excluded
        assert fig["sums_differ"] == 0, what
        assert fig.get("features_differ", 0) == 0, what
        if count:
            if ref["segments"] is not None:
                assert fig["render"]["segments"] == ref["segments"] and fig["trace"]["segments"] == ref["segments"], what
            if ref["counters"] is not None:
                for c in ("segments",) + KC.COUNTERS:
                    assert fig["render"][c] == ref["counters"][c] and fig["trace"][c] == ref["counters"][c], (what, c)
        assert len(set(launched)) == len(launched)
        assert set(launched) == want_launched, (what, sorted(set(launched) - want_launched), sorted(want_launched - set(launched)))
        if has_lists:
            assert tiles["list_launches"] > 0 and tiles["tiles"] == math.ceil(w / 8) * math.ceil(h / 8), (what, tiles)
        else:
            assert tiles["list_launches"] == 0, (what, tiles)
        return raw, got

    # ---- the drivers
    def drive(self, name, st, params, refused):
        P, g, walk = self.P, self.g, self.walk
        from path_tracer_ocaml_amd import abi
        assert params.size == 1
        w, h, depth = HS.W, HS.H, params.depth
        ref = HS.reference(walk.scene, st, depth, 1)
        xs, ys, ps = KC_samples(w, h)
        if name == "progressive":  # the error at K = 2, and a setter from inside its callback
            tried = []

            def on_update(k, rel_err, rgb, err):
                try:
                    g.set_lighting(0 if st.light else 1)
                    tried.append(None)
                except P.PtxError as e:
                    tried.append(e)
                return False
            rgb, err, done, _ = g.render_progressive(w, h, SPP, depth, 2, on_update=on_update, want_error=True)
            busy = HS.refusal("setter while a render runs")
            assert done == SPP and len(tried) == 2 and all(e is not None and HS.refused_as_documented(e, busy) for e in tried), tried
            assert _differ(rgb, HS.filmed(ref["sums"], st.film)) == 0, name
        elif name == "adaptive":  # T = 0: every pixel gets every pass
            rgb, _, passes, _ = g.render_adaptive(w, h, SPP, depth, 0.0, min_passes=2, passes_per_round=1)
            assert (passes == SPP).all()
            assert _differ(rgb, HS.filmed(ref["sums"], st.film)) == 0, name
        elif name == "pixels":  # a ragged list: every third pixel and the last
            pix = np.unique(np.concatenate([np.arange(0, w * h, 3), [w * h - 1]])).astype(np.int32)
            d_pix = self.torch.from_numpy(pix).to("cuda:0")
            raw = self.zeros(h, w, 3)
            g.render_pixels_device(P.render_params(w, h, SPP, depth), 0, SPP, d_pix.data_ptr(), len(pix), raw.data_ptr())
            raw = raw.cpu().numpy().reshape(-1, 3)
            assert _differ(raw[pix], ref["sums"].reshape(-1, 3)[pix]) == 0, name
            rest = np.setdiff1d(np.arange(w * h), pix)
            assert (_bits(raw[rest]) == 0).all(), name
        elif name == "features":  # in two slices; the plain check that follows compares one
            feat = self.zeros(h, w, 8)
            sliced = P.render_params(w, h, SPP, depth, passes_per_batch=2)
            g.render_features_device(sliced, 0, 2, feat.data_ptr())
            g.render_features_device(sliced, 2, SPP - 2, feat.data_ptr())
            if ref["features"] is not None:
                assert _differ(feat.cpu().numpy().reshape(-1, 8), ref["features"]) == 0, name
        elif name == "temporal":  # two frames onto the history, which is then dropped
            g.render_temporal(w, h, 4, depth, 0, 2)
            g.render_temporal(w, h, 4, depth, 2, 2)
            g.temporal_reset()
        elif name in ("render_rays", "intersect_rays", "walk_rays"):
            o, d = g.camera_rays(w, h, SPP, depth, xs, ys, ps)
            if name == "render_rays":  # the handle's own camera rays at the samples' offsets: the per-sample values
                offsets = ys.astype(np.int64) * w + xs + ps.astype(np.int64) * SPP
                got, _, _ = g.render_rays(o, d, offsets, max_bounces=depth)
                assert _differ(got, ref["want"]) == 0, name
            elif name == "intersect_rays":
                t, prim, _ = g.intersect_rays(o, d)
                assert (prim >= 0).any()
            else:
                walk_kind = abi.PTX_WALK_SHARED_ASM if KC.SCENES[walk.scene]["mode"] == "simd" else abi.PTX_WALK_SHARED_DIV
                t, prim = g.walk_rays(walk_kind, o, d)
                assert (prim >= 0).any()
        elif name == "ppm":
            from oracle import oracle as O
            lights = O.lights_cornell(w, h)
            pp = abi.ppm_params(w, h, iterations=1, max_bounces=2, photon_count=2000)
            if refused is None:
                img, _ = g.ppm_render(pp, lights)
                assert np.isfinite(img).all()
            else:
                with pytest.raises(P.PtxError) as err:
                    g.ppm_render(pp, lights)
                assert HS.refused_as_documented(err.value, refused), str(err.value)
        else:  # the replicas a handle owns follow its setters: two of them on this device, the sums gathered and filmed on the root
            assert name == "multi", name
            self.monkeypatch.setenv("PTX_MULTI_ALIAS", "1")  # test hook: replicas may share a device
            rgb, _ = g.render(w, h, SPP, depth, n_gpus=2, band_rows=4)
            assert _differ(rgb, HS.filmed(ref["sums"], st.film)) == 0, name

    def close(self):
        self.g.close()


_SAMPLES = {}


def KC_samples(w, h):
    import camera_pose_support as CP
    if (w, h) not in _SAMPLES:
        _SAMPLES[w, h] = CP.all_samples(w, h, SPP)
    return _SAMPLES[w, h]


@pytest.mark.parametrize("walk", HS.WALKS, ids=[w.name for w in HS.WALKS])
def test_a_handle_renders_its_state_whatever_its_history(P, torch, walk, monkeypatch):
    hd = Handle(P, torch, walk, monkeypatch)
    try:
        assert hd.g.stats()["traversal_in_lds"] == int(KC.SCENES[walk.scene]["lds"])
        before = hd.check(HS.START, HS.START_PARAMS, (walk.name, "start"))
        since_multi = None
        for i, (step, st, params, ref) in enumerate(HS.trace(walk)):
            what = (walk.name, i, step.kind, step.name, step.arg)
            if step.kind == "set":
                if ref is None:
                    HS.call_setter(hd.g, walk.scene, step)
                else:
                    with pytest.raises(P.PtxError) as err:
                        HS.call_setter(hd.g, walk.scene, step)
                    assert HS.refused_as_documented(err.value, ref), (what, str(err.value))
                if since_multi is not None:
                    since_multi += ref is None
            elif step.kind == "driver":
                if step.name == "multi":
                    assert since_multi is None or since_multi >= 3, what  # the later replica steps come after three state changes
                    since_multi = 0
                hd.drive(step.name, st, params, ref)
            assert HS.getters_differ(hd.g, walk.scene, st) == [], what
            now = hd.check(st, params, what)
            if step.kind == "set" and step.name == "film" and params.size == 1:  # the filmed image under the handle's film
                rgb, _ = hd.g.render(HS.W, HS.H, SPP, params.depth)
                assert _differ(rgb, HS.filmed(HS.reference(walk.scene, st, params.depth, 1)["sums"], st.film)) == 0, what
            if ref is not None:  # a refused call: the bits of the check before it
                assert _differ(now[0], before[0]) == 0 and _differ(now[1], before[1]) == 0, what
            before = now
    finally:
        hd.close()
