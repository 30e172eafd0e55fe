"""Sphere light sampling on the GPU (include/ptx.h, ptx_scene_set_sphere_light_sampling) against the restatement
tests/c/spherelight_oracle.c.

* the two diagnostics, ptx_light_sample / ptx_light_pdf -- the shade step's own device functions -- are the restatement bit for bit:
  2^16 inputs on a list of one sphere, of 64, and a mixed one; points at |f| = r (1 +- 2^-k), at the centre, r / d from 1 down to 1e-12,
  (u, v) at 0, at the top and denormal-small, directions on the cone's rim as sampled, f along every axis and its negation, picks
  that land on the last triangle and on the first sphere;
* per-sample radiance (ptx_trace_samples) in mode 2 with the option on is the restatement's bit for bit, 32 x 16, 20 000 samples, depths
  1, 2 and 8, PTX_FUSED=2 and PTX_FUSED=0 each in a fresh process: Shirley lit by a lamp sphere alone (Simd_leaf in LDS, and Array_leaf),
  cornell with its ceiling and a lamp sphere, a mesh walked from HBM / L2 with a lamp triangle pair and a lamp sphere, the three-way
  mixture under a sampled environment, and a camera inside one enclosing emissive sphere;
* on then off renders like a handle never touched: raw sums and the work counters of a counting render;
* the frame drivers agree with the per-sample values; a replica follows the setter.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

import spherelight_support as S
from test_spherelight_reference import LISTS, _numpy_table

pytestmark = pytest.mark.gpu
ROOT = S.ROOT
bits = S.bits


@pytest.fixture(scope="module")
def P():
    import path_tracer_ocaml_amd as P
    assert P.lib().ptx_device_count() >= 1, P.last_error()
    return P


# ------------------------------------------------------------------------------------------------ the diagnostics
def _diagnostic_inputs(tab, n, seed):
    """(points, uv, directions): the edge cases of the module's docstring, filled up to n with random ones"""
    rng = np.random.default_rng(seed)
    nt = len(tab.tri)
    axes = np.array([(1.0, 0, 0), (-1.0, 0, 0), (0, 1.0, 0), (0, -1.0, 0), (0, 0, 1.0), (0, 0, -1.0)])
    oblique = np.array([0.36, 0.48, 0.8])
    pts, uvs = [], []
    share = tab.sph[:, 5] / tab.total
    mid = (np.concatenate([[tab.tri[-1, 13]] if nt else [0.0], tab.sph[:-1, 6]]) + 0.5 * tab.sph[:, 5]) / tab.total  # x / W_total inside each sphere's span
    for s in (0, len(tab.sph) - 1):
        c, r = tab.sph[s, :3], tab.sph[s, 3]
        u_mid = 0.5 * mid[s]
        edge_uv = [(u, v) for u in (u_mid, 0.5 * (mid[s] - 0.5 * share[s]), 0.5 * (mid[s] + 0.5 * share[s]), 0.0, 0.5, 5e-324, 1e-310)
                   for v in (0.0, 1.0, 5e-324, 1e-310, 0.25, 1.0 - 2.0 ** -53)]
        k = np.arange(1, 53)
        for e in (oblique, axes[0], axes[5]):
            for sign in (1.0, -1.0):  # |f| = r (1 +- 2^-k)
                for kk in k:
                    pts.append(c + e * (r * (1.0 + sign * 2.0 ** -float(kk))))
                    uvs.append((u_mid, 0.3))
        for ratio in 10.0 ** -np.linspace(0.0, 12.0, 49):  # r / d from 1 down to 1e-12
            for e in (oblique, axes[2]):
                for uv in ((u_mid, 0.7), (0.5 * (mid[s] + 0.5 * share[s]), 0.7)):  # inside the cone, and on its rim
                    pts.append(c + e * (r / ratio))
                    uvs.append(uv)
        for uv in edge_uv:  # the centre, every axis and its negation (the frame rule's two special cases among them), just outside
            for p in [c.copy()] + [c - a * (3.0 * r) for a in axes] + [c - a * (1e6 * r) for a in axes]:
                pts.append(p)
                uvs.append(uv)
    if nt:  # picks that land on the last triangle and on the first sphere
        edge = 0.5 * (tab.tri[-1, 13] / tab.total)
        for u in (edge, np.nextafter(edge, 0.0), np.nextafter(edge, 1.0), edge * (1.0 - 1e-9), edge * (1.0 + 1e-9)):
            for v in (0.0, 0.4, 1.0 - 2.0 ** -53):
                pts.append(tab.sph[0, :3] + oblique * 0.7)
                uvs.append((u, v))
    pts, uvs = np.array(pts), np.array(uvs)
    m = n - len(pts)
    assert m > n // 2
    centres = tab.sph[:, :3]
    pick = rng.integers(0, len(centres), m)
    scale = np.where(rng.uniform(size=m) < 0.2, rng.uniform(0.0, 1.0, m), rng.uniform(1.0, 30.0, m))
    import envlight_support as ES
    rp = centres[pick] + ES.uniform_directions(m, seed + 1) * (tab.sph[pick, 3] * scale)[:, None]
    ruv = np.stack([rng.uniform(0.0, 0.5, m), rng.uniform(0.0, 1.0, m)], axis=1)
    return np.concatenate([pts, rp]), np.concatenate([uvs, ruv]), ES.uniform_directions(n, seed + 2)


@pytest.mark.parametrize("name", list(LISTS))
def test_diagnostics_equal_the_restatement(P, oracle, name):
    ptr, keep = LISTS[name](oracle)
    rest = S.Restatement(ptr, keep)
    tab = _numpy_table(rest)
    n = 1 << 16
    p, uv, dirs = _diagnostic_inputs(tab, n, 51)
    assert len(p) == n
    g = P.Scene(ptr, 0, keepalive=keep)
    g.set_sphere_light_sampling(True)
    g.set_lighting(2)
    got_d, got_k = g.light_sample(p, uv)
    want_d, want_k = rest.sample(p, uv)
    assert np.array_equal(got_k, want_k), name
    nbad = int((bits(got_d) != bits(want_d)).any(axis=1).sum())
    assert nbad == 0, f"{name}: {nbad} of {n} sampled directions differ"
    nt = len(tab.tri)
    if nt:
        assert (want_k == nt - 1).any() and (want_k == nt).any()
    assert (want_k == len(tab.cum) - 1).any()
    for probe in (dirs, want_d):  # arbitrary directions, and the sampled ones (the cone's rim among them)
        probe = np.where(np.isfinite(probe), probe, 0.0)
        got_p, want_p = g.light_pdf(p, probe), rest.pd(p, probe)
        nbad = int((bits(got_p) != bits(want_p)).sum())
        assert nbad == 0, f"{name}: {nbad} of {n} densities differ"
    g.close()


# ------------------------------------------------------------------------------------------------ per-sample radiance
def _child(tmp_path, env_extra):
    out = str(tmp_path / "child.npz")
    env = dict(os.environ)
    for k in ("PTX_FUSED", "PTX_BOUNCE_ORDER", "PTX_SOLO_ENTRIES", "PTX_FUSED_GLOBAL"):
        env.pop(k, None)
    env.update(env_extra)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "spherelight_gpu_child.py"), out], capture_output=True, text=True,
                       env=env, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    return np.load(out)


@pytest.fixture(scope="module")
def restated(oracle):
    """the restatement's radiance for the child's samples, per (scene, depth, option on), computed once"""
    cache, scenes = {}, {}
    xs, ys, ps = S.samples()

    def get(name, depth, on=True, mode=2):
        if name not in scenes:
            ptr, keep, _, _, env = S.descs(name)
            scenes[name] = (S.Restatement(ptr, keep), env)
        if (name, depth, on, mode) not in cache:
            rest, env = scenes[name]
            cache[(name, depth, on, mode)] = rest.trace_samples(mode, on, S.W, S.H, S.SPP, depth, xs, ys, ps, env=env,
                                                                env_sampling=env is not None and mode == 2)
        return cache[(name, depth, on, mode)]
    return get


@pytest.mark.parametrize("fused", ["2", "0"])
def test_samples_equal_the_restatement(tmp_path, restated, fused):
    got = _child(tmp_path, {"PTX_FUSED": fused})
    for name in S.SCENES:
        _, _, has_tris, in_lds, env = S.descs(name)
        if in_lds is not None:
            assert int(got[f"{name}/in_lds"]) == in_lds, name
        n_tri, n_sph = (int(v) for v in got[f"{name}/lights"])
        assert (n_tri > 0) == has_tris and n_sph == 1, name
        for depth in S.DEPTHS:
            g, c = got[f"{name}/{depth}"], restated(name, depth)
            assert g.shape == (S.N, 3) and S.N >= 20000
            nbad = int((bits(g) != bits(c)).any(axis=1).sum())
            assert nbad == 0, f"{name} depth {depth} PTX_FUSED={fused}: {nbad} of {S.N} samples differ"
            assert list(got[f"{name}/{depth}/launches"]) == [0, 0]  # carry_launches, solo_launches: a lit scene walks first
        # the option changes the estimator wherever a path outlives its first diffuse hit: against mode 2 with it off where that
        # mode has something else to sample, against path order where it has not
        other = restated(name, 8, on=False, mode=2 if (has_tris or env is not None) else 1)
        assert not np.array_equal(bits(got[f"{name}/8"]), bits(other)), name
        assert np.array_equal(bits(got[f"{name}/1"]), bits(restated(name, 1, on=False, mode=1))), name  # depth 1: no scatter is used
        assert float(got[f"{name}/8"].max()) > 0.0, name


def test_spheres_that_do_not_emit_leave_mode_2_as_it_is(P, oracle, restated):
    """the setter is refused on a scene without an emissive sphere, and the scene renders mode 2 as before"""
    ptr, keep, _, _, _ = S.descs("cornell_dark")
    g = P.Scene(ptr, 0, keepalive=keep)
    g.set_lighting(2)
    assert P.lib().ptx_scene_set_sphere_light_sampling(g._h, 1) == -1
    assert g.sphere_lights() == (False, 0, 0.0)
    xs, ys, ps = S.samples()
    got, _ = g.trace_samples(S.W, S.H, S.SPP, 8, xs, ys, ps)
    assert np.array_equal(bits(got), bits(restated("cornell_dark", 8, on=False)))
    g.close()


# ------------------------------------------------------------------------------------------------ on, then off
@pytest.mark.parametrize("name", ["shirley", "cornell"])
def test_on_then_off_is_a_handle_never_touched(P, oracle, name):
    torch = pytest.importorskip("torch")
    w, h, spp, depth = S.W, S.H, 6, 8
    ptr, keep, has_tris, _, _ = S.descs(name)
    fresh, touched = P.Scene(ptr, 0, keepalive=keep), P.Scene(ptr, 0, keepalive=keep)
    a = torch.zeros((h, w, 3), dtype=torch.float64, device="cuda:0")
    b = torch.zeros_like(a)
    touched.set_sphere_light_sampling(True)
    touched.set_lighting(2)
    touched.render_raw_device(P.render_params(w, h, spp, depth), b.data_ptr())
    on = b.cpu().numpy().copy()
    modes = (2, 1, 0) if has_tris else (1, 0)
    for mode in modes:
        touched.set_lighting(mode)
        if mode == modes[0]:
            touched.set_sphere_light_sampling(False)
        assert touched.sphere_lights() == (False, 0, 0.0)
        fresh.set_lighting(mode)
        for count in (False, True):
            params = P.render_params(w, h, spp, depth, count_work=count)
            sa = fresh.render_raw_device(params, a.data_ptr())
            sb = touched.render_raw_device(params, b.data_ptr())
            assert np.array_equal(bits(b.cpu().numpy()), bits(a.cpu().numpy())), (mode, count)
            if count:
                for key in ("samples", "segments", "nodes_tested", "prims_tested", "floor_tested"):
                    assert sa[key] == sb[key], (mode, key)
                assert sa["segments"] > sa["samples"] > 0
        assert not np.array_equal(bits(on), bits(a.cpu().numpy())), mode
    fresh.close()
    touched.close()


def test_the_setter_is_refused_while_a_render_runs(P):
    g = S.gpu_scene(P, "shirley", on=False, mode=1)
    seen = []

    def progress(n):
        seen.append(P.lib().ptx_scene_set_sphere_light_sampling(g._h, 1))
    g.render(S.W, S.H, 2, 4, progress=progress)
    assert seen and set(seen) == {-3}  # PTX_ERR_STATE
    assert g.sphere_lights() == (False, 0, 0.0)
    g.set_sphere_light_sampling(True)  # fine between renders
    g.close()


# ------------------------------------------------------------------------------------------------ frame drivers
@pytest.fixture(scope="module", params=["shirley", "cornell"])
def frame(P, request):
    w, h, n, depth = S.W, S.H, 12, 8
    g = S.gpu_scene(P, request.param)
    rgb, _ = g.render(w, h, n, depth)
    yield request.param, g, (w, h, n, depth), rgb.copy()
    g.close()


def test_raw_sums_and_a_pixel_list_sum_the_samples_in_pass_order(P, oracle, frame):
    torch = pytest.importorskip("torch")
    name, g, (w, h, n, depth), _ = frame
    import lighting_support as LS
    xs, ys, ps = LS.all_samples(w, h, n)
    ptr, keep, _, _, _ = S.descs(name)
    want = S.Restatement(ptr, keep).trace_samples(2, True, w, h, n, depth, xs, ys, ps).reshape(h * w, n, 3)
    sums = np.zeros((h * w, 3))
    for k in range(n):
        sums = sums + want[:, k]
    assert float(sums.max()) > 0.0
    raw = torch.zeros((h, w, 3), dtype=torch.float64, device="cuda:0")
    g.render_raw_device(P.render_params(w, h, n, depth), raw.data_ptr())
    assert np.array_equal(bits(raw.cpu().numpy().reshape(-1, 3)), bits(sums))
    # pass slices
    raw.zero_()
    params = P.render_params(w, h, n, depth, passes_per_batch=5)
    for first, count in ((0, 5), (5, 1), (6, 6)):
        g.render_passes_device(params, first, count, raw.data_ptr())
    assert np.array_equal(bits(raw.cpu().numpy().reshape(-1, 3)), bits(sums))
    # a pixel list: ragged, unordered
    pix = np.random.default_rng(9).choice(w * h, 37, replace=False).astype(np.int32)
    d_pix = torch.tensor(pix, device="cuda:0")
    raw.zero_()
    st = g.render_pixels_device(params, 0, n, d_pix.data_ptr(), len(pix), raw.data_ptr())
    got = raw.cpu().numpy().reshape(-1, 3)
    assert st["samples"] == len(pix) * n
    assert np.array_equal(bits(got[pix]), bits(sums[pix]))
    assert (got[np.setdiff1d(np.arange(w * h), pix)] == 0.0).all()


def test_progressive_and_adaptive_run_to_the_end_are_the_frame(P, frame):
    _, g, (w, h, n, depth), rgb = frame
    got, _, done, _ = g.render_progressive(w, h, n, depth, passes_per_update=5)
    assert done == n and np.array_equal(bits(got), bits(rgb))
    got, _, passes, _ = g.render_adaptive(w, h, n, depth, 0.0, min_passes=2, passes_per_round=3)
    assert (passes == n).all() and np.array_equal(bits(got), bits(rgb))


def test_bands_and_replicas_follow_the_setter(P, frame, monkeypatch):
    name, g, (w, h, n, depth), rgb = frame
    monkeypatch.setenv("PTX_MULTI_ALIAS", "1")
    # a replica made after the setter copies it
    r = g.replicate(0)
    assert r.sphere_lights() == g.sphere_lights() and r.sphere_lights()[0] and r.lighting()[0] == 2
    got, _ = P.render_multi([g, r], w, h, n, depth, band_rows=4)
    assert np.array_equal(bits(got), bits(rgb))
    r.close()
    # the replicas a scene owns (n_gpus = 2) are made before the next setter and follow it
    got, _ = g.render(w, h, n, depth, n_gpus=2, band_rows=4)
    assert np.array_equal(bits(got), bits(rgb))
    g.set_lighting(1)
    g.set_sphere_light_sampling(False)
    one, _ = g.render(w, h, n, depth)
    two, _ = g.render(w, h, n, depth, n_gpus=2, band_rows=4)
    assert np.array_equal(bits(one), bits(two)) and not np.array_equal(bits(one), bits(rgb))
    g.set_sphere_light_sampling(True)
    g.set_lighting(2)
    back, _ = g.render(w, h, n, depth, n_gpus=2, band_rows=4)
    assert np.array_equal(bits(back), bits(rgb))


# ------------------------------------------------------------------------------------------------ CLI
def test_cli_light_spheres(P, tmp_path):
    """shirley_spheres --sphere-lamp=... --lighting=sampled --light-spheres writes the PNG the same calls give through Python"""
    from path_tracer_ocaml_amd import host
    w, h, spp = 96, 48, 4
    lamp = (0.0, 4.0, 0.0, 0.5, 40.0)
    hs = host.shirley_lamp(w, h, lamp)
    g = P.Scene(hs.ptr, 0, keepalive=hs)
    g.set_lighting("path-order")
    plain, _ = g.render(w, h, spp, 8)
    g.set_sphere_light_sampling(True)
    g.set_lighting("sampled")
    assert g.sphere_lights()[:2] == (True, 1)
    want, _ = g.render(w, h, spp, 8)
    g.close()
    assert not np.array_equal(bits(want), bits(plain))
    host.write_png(str(tmp_path / "want.png"), want)
    out = tmp_path / "got.png"
    exe = os.path.join(ROOT, "path_tracer_ocaml_amd", "shirley_spheres")
    base = [exe, f"--dimension={w},{h}", f"--samples-per-pixel={spp}", "--no-progress", "-o", str(out)]
    r = subprocess.run(base + ["--sphere-lamp=" + ",".join(repr(v) for v in lamp), "--lighting=sampled", "--light-spheres"],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    assert out.read_bytes() == (tmp_path / "want.png").read_bytes()
    # without a lamp the library's refusal comes through, the count named
    r = subprocess.run(base + ["--lighting=sampled", "--light-spheres"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 1 and "ptx_scene_set_sphere_light_sampling" in r.stderr and "has 0" in r.stderr
