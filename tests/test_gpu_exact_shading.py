"""The kernels' shading against the interval restatement of tests/exact_shading.py, and against the oracle bit for bit:
ptx_debug_first_scatter and Scene.trace_samples (max_bounces 1 and 2) on the stock scenes (cornell's emissive
{path, emission} queue pairs among them), the shading soups and the designed families, over the per-bounce kernel
choices (PTX_FUSED 2 / 1 / 0), with and without the per-slot triangle frames (PTX_TRI_FRAME), and on the mesh walked
from HBM / L2 with and without k_bounce (PTX_FUSED_GLOBAL).  The switches are read when a scene is created, so they are
set before P.Scene()."""
import ctypes as C

import numpy as np
import pytest

import exact_shading as S

pytestmark = pytest.mark.gpu

_CACHE = {}


@pytest.fixture(scope="module")
def P():
    import path_tracer_ocaml_amd as P
    assert P.lib().ptx_device_count() >= 1, P.last_error()
    return P


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _i32(*a):
    return [np.ascontiguousarray(x, dtype=np.int32) for x in a]


def oracle_first_scatter(oracle, sc, W, H, spp, mb, xs, ys, ps):
    n = len(xs)
    ip, dp = oracle.ip, oracle.dp
    L = oracle.lib()
    L.orc_debug_first_scatter.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int64, ip, ip, ip, dp, dp, ip, ip]
    ray, att, alive, info = np.zeros((n, 6)), np.zeros((n, 3)), np.zeros(n, np.int32), np.zeros((n, 3), np.int32)
    xs, ys, ps = _i32(xs, ys, ps)
    L.orc_debug_first_scatter(sc._h, W, H, spp, mb, n, xs.ctypes.data_as(ip), ys.ctypes.data_as(ip), ps.ctypes.data_as(ip),
                              ray.ctypes.data_as(dp), att.ctypes.data_as(dp), alive.ctypes.data_as(ip), info.ctypes.data_as(ip))
    return ray, att, alive, info


def ptx_first_scatter(P, g, W, H, spp, mb, xs, ys, ps):
    from path_tracer_ocaml_amd import abi
    n = len(xs)
    ip, dp = P.ip, P.dp
    G = P.lib()
    G.ptx_debug_first_scatter.argtypes = [C.c_void_p, C.POINTER(abi.RenderParams), C.c_int64, ip, ip, ip, dp, dp, ip]
    ray, att, alive = np.zeros((n, 6)), np.zeros((n, 3)), np.zeros(n, np.int32)
    xs, ys, ps = _i32(xs, ys, ps)
    params = P.render_params(W, H, spp, mb)
    rc = G.ptx_debug_first_scatter(g._h, C.byref(params), n, xs.ctypes.data_as(ip), ys.ctypes.data_as(ip), ps.ctypes.data_as(ip),
                                   ray.ctypes.data_as(dp), att.ctypes.data_as(dp), alive.ctypes.data_as(ip))
    assert rc == 0, P.last_error()
    return ray, att, alive


def case(name, oracle, mb):
    """The description, the restated samples at max_bounces mb and the oracle's results, built once per module."""
    key = (name, mb)
    if key not in _CACHE:
        from path_tracer_ocaml_amd import abi
        if name in S.FAMILIES:
            ptr, keep, W, H, spp, xs, ys, ps = S.family_desc(name, oracle, abi)
        else:
            ptr, keep, W, H, spp = S.stock_desc(name, oracle, abi)
            xs, ys, ps = S.random_samples(name, W, H, spp, n=1500 if name == "ganesha_150k" else 3000)
        tab = S.Tables(ptr)
        smp = S.Samples(oracle, tab, W, H, spp, mb, xs, ys, ps)
        sc = oracle.Scene(ptr, keep)
        fs = oracle_first_scatter(oracle, sc, W, H, spp, 2, xs, ys, ps) if mb == 2 else None
        rgb, _ = sc.trace_samples(W, H, spp, mb, xs, ys, ps)
        _CACHE[key] = (ptr, keep, smp, fs, rgb, (W, H, spp, xs, ys, ps))
    return _CACHE[key]


def _first_scatter_check(P, oracle, name):
    ptr, keep, smp, (c_ray, c_att, c_alive, info), _, (W, H, spp, xs, ys, ps) = case(name, oracle, 2)
    g = P.Scene(ptr, 0, keepalive=keep)
    try:
        ray, att, alive = ptx_first_scatter(P, g, W, H, spp, 2, xs, ys, ps)
    finally:
        g.close()
    assert np.array_equal(alive, c_alive), f"{int((alive != c_alive).sum())} samples alive on one side only"
    live = c_alive == 1
    assert np.array_equal(bits(ray[live]), bits(c_ray[live])), "next ray differs from the oracle"
    assert np.array_equal(bits(att[live]), bits(c_att[live])), "attenuation differs from the oracle"
    bad, summ, _, _ = S.check_first_scatter(smp, ray, att, alive)
    print(f"\n{name}: {summ}")
    assert not bad, "\n".join(bad)


SCENES = S.STOCK + list(S.FAMILIES)


@pytest.mark.parametrize("tri_frame", [1, 0])
@pytest.mark.parametrize("fused", [2, 1, 0])
@pytest.mark.parametrize("name", SCENES)
def test_first_scatter_equals_oracle_and_restatement(P, oracle, name, fused, tri_frame, monkeypatch):
    monkeypatch.setenv("PTX_FUSED", str(fused))
    monkeypatch.setenv("PTX_TRI_FRAME", str(tri_frame))
    _first_scatter_check(P, oracle, name)


@pytest.mark.parametrize("fused_global", [1, 0])
def test_mesh_first_scatter_equals_oracle_and_restatement(P, oracle, fused_global, monkeypatch):
    """The ganesha-like mesh at 150k triangles is walked from HBM / L2: k_bounce (1) or k_trace + k_shade_pool (0)."""
    monkeypatch.setenv("PTX_FUSED_GLOBAL", str(fused_global))
    _first_scatter_check(P, oracle, "ganesha_150k")


# the families are solved on the camera rays of max_bounces 2 and run at that depth only
RADIANCE_CASES = [(n, mb) for n in S.STOCK for mb in (1, 2)] + [(n, S.FAMILY_MB) for n in S.FAMILIES]


@pytest.mark.parametrize("tri_frame", [1, 0])
@pytest.mark.parametrize("name,mb", RADIANCE_CASES)
def test_radiance_equals_oracle_and_restatement(P, oracle, name, mb, tri_frame, monkeypatch):
    """Scene.trace_samples: bit for bit the oracle's, and inside the restated enclosure (for 2, chained on the next ray
    of the first scatter, which must itself lie inside its enclosure)."""
    monkeypatch.setenv("PTX_TRI_FRAME", str(tri_frame))
    ptr, keep, smp, fs, c_rgb, (W, H, spp, xs, ys, ps) = case(name, oracle, mb)
    g = P.Scene(ptr, 0, keepalive=keep)
    try:
        rgb, _ = g.trace_samples(W, H, spp, mb, xs, ys, ps)
        fsg = ptx_first_scatter(P, g, W, H, spp, 2, xs, ys, ps) if mb == 2 else None
    finally:
        g.close()
    assert np.array_equal(bits(rgb), bits(c_rgb)), f"{int((bits(rgb) != bits(c_rgb)).any(1).sum())} samples differ from the oracle"
    if mb == 2:
        ray, att, alive = fsg
        bad, _, _, _ = S.check_first_scatter(smp, ray, att, alive)
        assert not bad, "\n".join(bad)
        target = S.FAMILIES.get(name, "")
        bad, summ, _ = S.check_radiance(smp, rgb, ray[:, :3], ray[:, 3:], target=target if target.endswith("_2") else None)
    else:
        bad, summ, _ = S.check_radiance(smp, rgb)
    print(f"\n{name} max_bounces {mb}: {summ}")
    assert not bad, "\n".join(bad)
