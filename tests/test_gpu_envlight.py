"""Environment sampling on the GPU (include/ptx.h, ptx_scene_set_environment_sampling) against the restatement
tests/c/envlight_oracle.c.

* the two diagnostics, ptx_environment_sample / ptx_environment_pdf -- the shade step's own device functions -- are the restatement
  bit for bit: 2^16 inputs each on every image of the density-table list, nearest and bilinear, identity and a rotation, the edge
  values of (a, b), poles, axes and directions with a zero component;
* per-sample radiance (ptx_trace_samples) in mode 2 with sampling on is the restatement's bit for bit: Shirley (Simd_leaf in LDS, and
  Array_leaf) lit by the environment alone, a small open triangle scene with a lamp in LDS and a mesh walked from HBM / L2 with both
  lists; depths 1, 2, 8; PTX_FUSED=2 and PTX_FUSED=0, each in a fresh process; every one of the 20 000 samples is compared;
* sampling on then off leaves a scene that renders like one never touched;
* the frame drivers agree with each other and with the per-sample results; replicas follow the setter.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

import envlight_support as S

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
bits = S.bits


@pytest.fixture(scope="module")
def P():
    import path_tracer_ocaml_amd as P
    assert P.lib().ptx_device_count() >= 1, P.last_error()
    return P


# ------------------------------------------------------------------------------------------------ the diagnostics
@pytest.mark.parametrize("name", list(S.table_images()))
def test_diagnostics_equal_the_restatement(P, oracle, name):
    img = S.table_images()[name]
    rng = np.random.default_rng(41)
    n = 1 << 16
    ab = np.concatenate([S.edge_pairs(), rng.uniform(0.0, 1.0, (n - 16, 2))])
    dirs = np.concatenate([S.edge_directions(), S.uniform_directions(n - len(S.edge_directions()), 42)])
    d = oracle.desc_shirley(32, 16)
    g = P.Scene(d.ptr, 0, keepalive=d)
    for bilinear in (False, True):
        for R in (None, S.rotation([0.3, 1.0, 0.2], 50.0)):
            g.set_environment(img, R, bilinear=bilinear)
            g.set_environment_sampling(True)
            got_d, got_t = g.environment_sample(ab)
            want_d, want_t = S.c_sample(img, R, ab)
            assert np.array_equal(got_t, want_t), (name, bilinear, R is None)
            assert int((bits(got_d) != bits(want_d)).any(axis=1).sum()) == 0, (name, bilinear, R is None)
            for probe in (dirs, want_d):  # arbitrary directions, and the sampled ones (texel edges)
                got_p = g.environment_pdf(probe)
                want_p, _ = S.c_pd(img, R, probe)
                assert int((bits(got_p) != bits(want_p)).sum()) == 0, (name, bilinear, R is None)
            assert np.isfinite(got_d).all() and (want_p >= 0.0).all()
    g.close()


# ------------------------------------------------------------------------------------------------ per-sample radiance
def _child(tmp_path, env_extra):
    out = str(tmp_path / "child.npz")
    env = dict(os.environ)
    for k in ("PTX_FUSED", "PTX_BOUNCE_ORDER", "PTX_SOLO_ENTRIES", "PTX_FUSED_GLOBAL"):
        env.pop(k, None)
    env.update(env_extra)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "envlight_gpu_child.py"), out], capture_output=True, text=True,
                       env=env, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    return np.load(out)


@pytest.fixture(scope="module")
def restated(oracle):
    """the restatement's radiance for the child's samples, per (scene, depth, sampling, mode), computed once"""
    cache, scenes = {}, {}
    xs, ys, ps = S.samples()
    img, flags, R = S.environment()

    def get(name, depth, sampling=True, mode=2):
        if name not in scenes:
            ptr, keep, _, _ = S.descs(name)
            scenes[name] = S.Restatement(ptr, keep)
        if (name, depth, sampling, mode) not in cache:
            cache[(name, depth, sampling, mode)] = scenes[name].trace_samples(img, flags, R, mode, sampling, S.W, S.H, S.SPP, depth, xs, ys, ps)
        return cache[(name, depth, sampling, mode)]
    return get


@pytest.mark.parametrize("fused", ["2", "0"])
def test_samples_equal_the_restatement(tmp_path, restated, fused):
    got = _child(tmp_path, {"PTX_FUSED": fused})
    for name in S.SCENES:
        _, _, has_lights, in_lds = S.descs(name)
        if in_lds is not None:
            assert int(got[f"{name}/in_lds"]) == in_lds, name
        assert (int(got[f"{name}/lights"]) > 0) == has_lights, name
        for depth in S.DEPTHS:
            g, c = got[f"{name}/{depth}"], restated(name, depth)
            assert g.shape == (S.N, 3) and S.N >= 20000
            nbad = int((bits(g) != bits(c)).any(axis=1).sum())
            assert nbad == 0, f"{name} depth {depth} PTX_FUSED={fused}: {nbad} of {S.N} samples differ"
            assert list(got[f"{name}/{depth}/launches"]) == [0, 0]  # carry_launches, solo_launches
        # sampling changes the estimator wherever a path outlives its first diffuse hit
        assert not np.array_equal(bits(got[f"{name}/8"]), bits(restated(name, 8, sampling=False, mode=2 if has_lights else 1))), name
        assert float(got[f"{name}/8"].max()) > 0.0, name


# ------------------------------------------------------------------------------------------------ on, then off
@pytest.mark.parametrize("name", ["shirley", "open_lamp"])
def test_sampling_on_then_off_is_a_scene_never_touched(P, oracle, name):
    torch = pytest.importorskip("torch")
    w, h, spp, depth = S.W, S.H, 6, 8
    ptr, keep, has_lights, _ = S.descs(name)
    img, flags, R = S.environment()
    params = P.render_params(w, h, spp, depth)
    fresh, touched = P.Scene(ptr, 0, keepalive=keep), P.Scene(ptr, 0, keepalive=keep)
    a = torch.zeros((h, w, 3), dtype=torch.float64, device="cuda:0")
    b = torch.zeros_like(a)
    for g in (fresh, touched):
        g.set_environment(img, R)
    touched.set_environment_sampling(True)
    touched.set_lighting(2)
    touched.render_raw_device(params, b.data_ptr())
    on = b.cpu().numpy().copy()
    modes = (2, 0) if has_lights else (0,)
    for mode in modes:
        touched.set_lighting(mode)
        if mode == modes[0]:
            touched.set_environment_sampling(False)
        assert touched.environment_sampling() == (False, 0.0)
        fresh.set_lighting(mode)
        fresh.render_raw_device(params, a.data_ptr())
        touched.render_raw_device(params, b.data_ptr())
        assert np.array_equal(bits(b.cpu().numpy()), bits(a.cpu().numpy())), mode
        assert not np.array_equal(bits(on), bits(a.cpu().numpy())), mode
    fresh.close()
    touched.close()


def test_the_setter_is_refused_while_a_render_runs(P):
    g = S.gpu_scene(P, "shirley", sampling=False, mode=0, w=64, h=32)
    seen = []

    def progress(n):
        seen.append(P.lib().ptx_scene_set_environment_sampling(g._h, 1))
    g.render(64, 32, 2, 4, progress=progress)
    assert seen and set(seen) == {-3}  # PTX_ERR_STATE
    assert g.environment_sampling() == (False, 0.0)
    g.set_environment_sampling(True)  # fine between renders
    g.close()


# ------------------------------------------------------------------------------------------------ frame drivers
@pytest.fixture(scope="module", params=["shirley", "open_lamp"])
def sun_frame(P, request):
    w, h, n, depth = S.W, S.H, 12, 8
    g = S.gpu_scene(P, request.param)
    rgb, _ = g.render(w, h, n, depth)
    yield request.param, g, (w, h, n, depth), rgb.copy()
    g.close()


def test_pass_slices_sum_the_samples_in_pass_order(P, oracle, sun_frame):
    torch = pytest.importorskip("torch")
    name, g, (w, h, n, depth), _ = sun_frame
    raw = torch.zeros((h, w, 3), dtype=torch.float64, device="cuda:0")
    params = P.render_params(w, h, n, depth, passes_per_batch=5)
    for first, count in ((0, 5), (5, 1), (6, 6)):
        g.render_passes_device(params, first, count, raw.data_ptr())
    raw = raw.cpu().numpy()
    rng = np.random.default_rng(5)
    pix = rng.choice(w * h, 64, replace=False)
    px, py = pix % w, pix // w
    xs, ys, ps = np.repeat(px, n), np.repeat(py, n), np.tile(np.arange(n), 64)
    ptr, keep, _, _ = S.descs(name)
    img, flags, R = S.environment()
    want = S.Restatement(ptr, keep).trace_samples(img, flags, R, 2, True, w, h, n, depth, xs, ys, ps).reshape(64, n, 3)
    sums = np.zeros((64, 3))
    for k in range(n):
        sums = sums + want[:, k]
    assert np.array_equal(bits(raw[py, px]), bits(sums))
    assert float(sums.max()) > 0.0


def test_progressive_run_to_the_end_is_the_frame(P, sun_frame):
    _, g, (w, h, n, depth), rgb = sun_frame
    got, _, done, _ = g.render_progressive(w, h, n, depth, passes_per_update=5)
    assert done == n
    assert np.array_equal(bits(got), bits(rgb))


def test_replicas_follow_the_setter(P, sun_frame, monkeypatch):
    name, g, (w, h, n, depth), rgb = sun_frame
    monkeypatch.setenv("PTX_MULTI_ALIAS", "1")
    # a replica made after the setter copies it
    r = g.replicate(0)
    assert r.environment_sampling() == g.environment_sampling() and r.environment_sampling()[0] and r.lighting()[0] == 2
    got, _ = P.render_multi([g, r], w, h, n, depth)
    assert np.array_equal(bits(got), bits(rgb))
    r.close()
    # the replicas a scene owns (n_gpus = 2) are made before the next setter and follow it
    got, _ = g.render(w, h, n, depth, n_gpus=2)
    assert np.array_equal(bits(got), bits(rgb))
    img, flags, R = S.environment()
    other = S.sun_sky(sun=(10, 25), seed=6)
    g.set_environment(other, R)  # rebuilds the density, on the replicas too
    one, _ = g.render(w, h, n, depth)
    two, _ = g.render(w, h, n, depth, n_gpus=2)
    assert np.array_equal(bits(one), bits(two)) and not np.array_equal(bits(one), bits(rgb))
    g.set_environment(img, R)
    back, _ = g.render(w, h, n, depth, n_gpus=2)
    assert np.array_equal(bits(back), bits(rgb))


# ------------------------------------------------------------------------------------------------ CLI
def test_cli_envmap_sample(P, tmp_path):
    """shirley_spheres --envmap=... --lighting=sampled --envmap-sample writes the PNG the same calls give through Python"""
    import ctypes as C
    from path_tracer_ocaml_amd import host
    from test_pfm import write_pfm
    env = S.sun_sky(32, 16, sun=(20, 11)).astype(np.float32)
    write_pfm(tmp_path / "env.pfm", env, little=False)
    w, h, spp = 96, 48, 4
    R = (C.c_double * 9)()
    host.lib().pth_rotation_y.argtypes = [C.c_double, C.POINTER(C.c_double)]
    host.lib().pth_rotation_y(40.0, R)
    hs = host.shirley_spheres(w, h)
    g = P.Scene(hs.ptr, 0, keepalive=hs)
    g.set_environment(env.astype(np.float64), rotation=np.array(list(R)))
    plain, _ = g.render(w, h, spp, 8)
    g.set_environment_sampling(True)
    g.set_lighting("sampled")
    want, _ = g.render(w, h, spp, 8)
    g.close()
    assert not np.array_equal(bits(want), bits(plain))
    host.write_png(str(tmp_path / "want.png"), want)
    out = tmp_path / "got.png"
    r = subprocess.run([os.path.join(ROOT, "path_tracer_ocaml_amd", "shirley_spheres"), f"--dimension={w},{h}", f"--samples-per-pixel={spp}",
                        "--no-progress", f"--envmap={tmp_path / 'env.pfm'}", "--envmap-rotate=40", "--lighting=sampled", "--envmap-sample",
                        "-o", str(out)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert out.read_bytes() == (tmp_path / "want.png").read_bytes()
