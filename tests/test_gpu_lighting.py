"""Lighting modes 1 (path order) and 2 (sampled) on the GPU against the restatement tests/c/lighting_oracle.c.

* per-sample radiance (ptx_trace_samples) is the restatement's bit for bit: stock cornell, the lamp scene, a mesh walked from
  HBM / L2 with a lamp; depths 1, 2, 8, 16; the one-kernel-per-bounce schedule (PTX_FUSED=2) and the two-kernel one (PTX_FUSED=0),
  each in a fresh process; every one of the 20 000 samples of a case is compared;
* a lit scene takes the walk-first kernel even where the shade-first one is forced (PTX_BOUNCE_ORDER=1), and goes back to it
  when the mode does;
* mode 0 after set and reset is a never-touched scene bit for bit;
* the frame-level drivers in mode 2 agree with each other and with the per-sample results.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

import lighting_support as S
import lighting_gpu_child as CH

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


@pytest.fixture(scope="module")
def P():
    import path_tracer_ocaml_amd as P
    assert P.lib().ptx_device_count() >= 1, P.last_error()
    return P


def _child(tmp_path, env_extra, *flags):
    out = str(tmp_path / "child.npz")
    env = dict(os.environ)
    for k in ("PTX_FUSED", "PTX_BOUNCE_ORDER", "PTX_SOLO_ENTRIES", "PTX_FUSED_GLOBAL"):
        env.pop(k, None)
    env.update(env_extra)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "lighting_gpu_child.py"), out, *flags], capture_output=True,
                       text=True, env=env, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    return np.load(out)


@pytest.fixture(scope="module")
def restated(oracle):
    """the restatement's radiance for the child's samples, per (scene, mode, depth), computed once"""
    cache, scenes = {}, {}
    xs, ys, ps = CH.samples()

    def get(name, mode, depth):
        if name not in scenes:
            d, keep = CH.descs(name)
            import ctypes
            scenes[name] = S.Restatement(d if isinstance(d, ctypes.POINTER(S.abi.SceneDesc)) else ctypes.pointer(d), keep)
        if (name, mode, depth) not in cache:
            cache[(name, mode, depth)] = scenes[name].trace_samples(mode, CH.W, CH.H, CH.SPP, depth, xs, ys, ps)
        return cache[(name, mode, depth)]
    return get


@pytest.mark.parametrize("fused", ["2", "0"])
def test_samples_equal_the_restatement(tmp_path, restated, fused):
    got = _child(tmp_path, {"PTX_FUSED": fused})
    assert int(got["cornell/in_lds"]) == 1 and int(got["lamp003/in_lds"]) == 1
    assert int(got["mesh/in_lds"]) == 0  # >= 4000 triangles: walked from HBM / L2
    for name in CH.SCENES:
        for mode in (1, 2):
            for depth in CH.DEPTHS:
                g, c = got[f"{name}/{mode}/{depth}"], restated(name, mode, depth)
                assert g.shape == (CH.N, 3) and CH.N >= 20000
                nbad = int((bits(g) != bits(c)).any(axis=1).sum())
                assert nbad == 0, f"{name} mode {mode} depth {depth} PTX_FUSED={fused}: {nbad} of {CH.N} samples differ"
                assert list(got[f"{name}/{mode}/{depth}/launches"]) == [0, 0]
            # the two modes are different estimators wherever a path outlives its first diffuse hit
        assert not np.array_equal(bits(got[f"{name}/1/8"]), bits(got[f"{name}/2/8"])), name
        assert float(got[f"{name}/2/8"].max()) > 0.0, name


def test_a_lit_scene_takes_the_walk_first_kernel(tmp_path, restated):
    got = _child(tmp_path, {"PTX_FUSED": "2", "PTX_BOUNCE_ORDER": "1"}, "--carry")
    for mode in (1, 2):
        for depth in CH.DEPTHS:
            g, c = got[f"cornell/{mode}/{depth}"], restated("cornell", mode, depth)
            assert int((bits(g) != bits(c)).any(axis=1).sum()) == 0, (mode, depth)
        assert list(got[f"frame/{mode}"]) == [0, 0], mode  # carry_launches, solo_launches
    assert int(got["frame/0"][0]) > 0  # back in mode 0 the shade-first kernel runs again


def test_mode_0_is_restored(P, oracle):
    torch = pytest.importorskip("torch")
    w = h = 128
    spp, depth = 8, 8
    hs = S.host_scene("lamp012", w, h)
    params = P.render_params(w, h, spp, depth)
    fresh, touched = P.Scene(hs.ptr, 0, keepalive=hs), P.Scene(hs.ptr, 0, keepalive=hs)
    a = torch.zeros((h, w, 3), dtype=torch.float64, device="cuda:0")
    b = torch.zeros_like(a)
    fresh.render_raw_device(params, a.data_ptr())
    lit = {}
    for mode in (2, 1):
        touched.set_lighting(mode)
        touched.render_raw_device(params, b.data_ptr())
        lit[mode] = b.cpu().numpy().copy()
        assert not np.array_equal(bits(lit[mode]), bits(a.cpu().numpy())), mode
    touched.set_lighting(0)
    assert touched.lighting()[0] == 0
    touched.render_raw_device(params, b.data_ptr())
    assert np.array_equal(bits(b.cpu().numpy()), bits(a.cpu().numpy()))
    c = oracle.Scene(hs.ptr, hs).render(w, h, spp, depth, threads=8, want_raw=True)
    assert np.array_equal(bits(a.cpu().numpy()), bits(c["raw"]))
    fresh.close()
    touched.close()


def test_set_lighting_is_refused_while_a_render_runs(P):
    hs = S.host_scene("lamp003", 64, 64)
    g = P.Scene(hs.ptr, 0, keepalive=hs)
    seen = []

    def progress(n):
        seen.append(P.lib().ptx_scene_set_lighting(g._h, 2))
    g.render(64, 64, 2, 4, progress=progress)
    assert seen and set(seen) == {-3}  # PTX_ERR_STATE
    assert g.lighting()[0] == 0
    g.set_lighting(2)  # fine between renders
    g.close()


@pytest.fixture(scope="module")
def lamp_frame(P):
    """the lamp scene in mode 2 and its plain frame"""
    w, h, n, depth = 96, 64, 12, 8
    hs = S.host_scene("lamp003", w, h)
    g = P.Scene(hs.ptr, 0, keepalive=hs)
    g.set_lighting("sampled")
    rgb, _ = g.render(w, h, n, depth)
    yield hs, g, (w, h, n, depth), rgb.copy()
    g.close()


def test_pass_slices_sum_the_samples_in_pass_order(P, lamp_frame):
    torch = pytest.importorskip("torch")
    hs, g, (w, h, n, depth), _ = lamp_frame
    raw = torch.zeros((h, w, 3), dtype=torch.float64, device="cuda:0")
    params = P.render_params(w, h, n, depth, passes_per_batch=5)
    for first, count in ((0, 5), (5, 1), (6, 6)):
        g.render_passes_device(params, first, count, raw.data_ptr())
    raw = raw.cpu().numpy()
    rng = np.random.default_rng(5)
    pix = rng.choice(w * h, 64, replace=False)
    px, py = pix % w, pix // w
    xs, ys, ps = np.repeat(px, n), np.repeat(py, n), np.tile(np.arange(n), 64)
    want = S.Restatement(hs.ptr, hs).trace_samples(2, w, h, n, depth, xs, ys, ps).reshape(64, n, 3)
    sums = np.zeros((64, 3))
    for k in range(n):
        sums = sums + want[:, k]
    assert np.array_equal(bits(raw[py, px]), bits(sums))
    assert float(sums.max()) > 0.0


def test_progressive_run_to_the_end_is_the_frame(P, lamp_frame):
    _, g, (w, h, n, depth), rgb = lamp_frame
    got, _, done, _ = g.render_progressive(w, h, n, depth, passes_per_update=5)
    assert done == n
    assert np.array_equal(bits(got), bits(rgb))


def test_adaptive_at_target_zero_is_the_frame(P, lamp_frame):
    _, g, (w, h, n, depth), rgb = lamp_frame
    got, _, passes, _ = g.render_adaptive(w, h, n, depth, 0.0, min_passes=4, passes_per_round=3)
    assert (passes == n).all()
    assert np.array_equal(bits(got), bits(rgb))


def test_two_aliased_replicas_render_the_frame(P, lamp_frame, monkeypatch):
    _, g, (w, h, n, depth), rgb = lamp_frame
    monkeypatch.setenv("PTX_MULTI_ALIAS", "1")
    r = g.replicate(0)
    assert r.lighting()[:2] == (2, 2)  # ptx_scene_replicate copies the mode
    got, _ = P.render_multi([g, r], w, h, n, depth)
    assert np.array_equal(bits(got), bits(rgb))
    r.close()
