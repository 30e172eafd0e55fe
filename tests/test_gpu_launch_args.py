"""The two calls that launch k_trace outside the bounce loop, after a render on the same handle: ptx_intersect_rays and
ptx_render_features_device take the bounce number and the parked-walk buffer as arguments of the launch, so neither may depend on
what the render before them left behind.  Run with PTX_BOUNCE_PACKET=2, where a bounce number decides between two kernels, in a
fresh process (tests/launch_args_gpu_child.py), on stock Shirley (Simd_leaf) and cornell (Array_leaf), both LDS-resident.

* ptx_intersect_rays on 256 camera rays of the frame: primitive, t bit for bit and the work counters are the oracle's.
* ptx_render_features_device for the frame (32 x 16, 2 passes, depth 3): per pass, hits and depth are the oracle's closest hit of
  the oracle's camera ray bit for bit, normal and albedo lie inside the enclosures of tests/feature_reference.py and a miss shows
  the background -- the reference of tests/test_gpu_features.py, here for every sample of the frame; the sums of both passes are
  the sequential binary64 sum of the single passes, bit for bit.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

import exact_shading as S
import feature_reference as FR
import launch_args_gpu_child as CH

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


@pytest.fixture(scope="module")
def got(tmp_path_factory):
    pytest.importorskip("torch")
    out = str(tmp_path_factory.mktemp("launch_args") / "child.npz")
    env = dict(os.environ)
    for k in ("PTX_FUSED", "PTX_BOUNCE_ORDER", "PTX_SOLO_ENTRIES", "PTX_FUSED_GLOBAL", "PTX_PRIMARY_WALK", "PTX_TRACE_BLOCK"):
        env.pop(k, None)
    env["PTX_BOUNCE_PACKET"] = "2"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "launch_args_gpu_child.py"), out], capture_output=True, text=True,
                       env=env, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    return np.load(out)


@pytest.fixture(scope="module")
def reference(oracle):
    """per scene, computed once: the frame's samples, their camera rays and exact closest hits, the enclosures of the feature
    record, and the oracle's answer to the child's rays"""
    from path_tracer_ocaml_amd import abi
    cache = {}

    def get(name):
        if name not in cache:
            ptr, keep, _, _, _ = S.stock_desc(name, oracle, abi)
            xs, ys, ps = CH.samples()
            smp = S.Samples(oracle, S.Tables(ptr), CH.W, CH.H, CH.SPP, CH.DEPTH, xs, ys, ps)
            assert np.array_equal(bits(smp.D), bits(CH.camera_rays(oracle, ptr, xs, ys, ps)))
            sc = oracle.Scene(ptr, keep)
            t, prim, _ = sc.intersect_rays(smp.O, smp.D)
            D = smp.D[:CH.N_RAYS]
            t_rays, prim_rays, ct = sc.intersect_rays(np.zeros_like(D), D)
            sc.close()
            cache[name] = dict(xs=xs, ys=ys, ps=ps, t=t, prim=prim, enc=FR.enclosures(smp), t_rays=t_rays, prim_rays=prim_rays, ct=ct)
        return cache[name]
    return get


@pytest.mark.parametrize("name", CH.SCENES)
def test_intersect_rays_after_a_render(got, reference, name):
    r = reference(name)
    assert int(got[f"{name}/in_lds"]) == 1 and got[f"{name}/rgb"].max() > 0.0  # the render before it: depth 3, bounces 1 and 2 queued
    assert np.array_equal(got[f"{name}/prim"], r["prim_rays"]) and (r["prim_rays"] >= 0).any()
    assert np.array_equal(bits(got[f"{name}/t"]), bits(r["t_rays"]))
    assert list(got[f"{name}/counters"]) == [r["ct"][k] for k in CH.COUNTERS]


@pytest.mark.parametrize("name", CH.SCENES)
def test_features_after_a_render(got, reference, name):
    r = reference(name)
    xs, ys, ps, enc = r["xs"], r["ys"], r["ps"], r["enc"]
    singles = np.stack([got[f"{name}/feat/pass{p}"] for p in range(CH.SPP)])
    rec = singles[ps, ys, xs]
    hit = r["prim"] >= 0
    assert hit.any()
    assert np.array_equal(rec[:, 7], hit.astype(np.float64))
    assert np.array_equal(bits(rec[hit, 6]), bits(r["t"][hit]))
    assert (rec[~hit, 6] == 0.0).all() and (rec[~hit, 3:6] == 0.0).all()
    rob = enc["robust"]
    assert int((~rob).sum()) <= len(rob) // 100
    assert np.array_equal(enc["hit"][rob], hit[rob])
    h, m = rob & hit, rob & ~hit
    assert not (h & ~S.inside(enc["normal"], rec[:, 3:6])).any()
    assert np.array_equal(bits(rec[h, 0:3]), bits(enc["albedo"][h]))
    assert not (m & ~S.inside(enc["bg"], rec[:, 0:3])).any()
    want = np.zeros((CH.H, CH.W, 8))
    for p in range(CH.SPP):
        want = want + singles[p]
    assert np.array_equal(bits(got[f"{name}/feat/whole"]), bits(want))
