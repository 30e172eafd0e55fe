"""Renders with the dynamic LDS buffer NEARLY FULL, and just past full: what the stock scenes never reach.

For Simd_leaf spheres, Array_leaf spheres and a triangle soup (the generators of tests/test_gpu_fuzz.py, one fixed soup each, taken
a prefix at a time) the size is bisected at which csrc/pt_lds_layout.h stops calling the scene LDS-resident: host-only scenes
(device -1) give tree size, depth and slot count, the `layout` mode of tests/c/asan_host_driver.cpp -- built here WITHOUT the
sanitizers, a plain host program -- gives the placement and every kernel's layout for those integers.  The largest resident prefix,
the next one (not resident) and the largest prefix that still keeps the binary64 bounds in LDS are rendered 64 x 64, spp 2, depth 5 -- 128 chunks, four 1024-thread workgroups: pools fill and
walks are parked -- under the switches that reach a different kernel or region, and compared with the oracle: raw sums and the work
counters bit for bit.  What ran (traversal_in_lds, carry launches, k_bounce or the two kernels) must be what the layout said.

k_bounce_carry's larger parked record never stops fitting first: behind an image that k_trace admits (80 KiB with its stacks) its
launch stays far below PT_LDS_BOUNCE_LIMIT at these depths; the test asserts that of every resident scene instead of assuming it."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

from test_gpu_edge_cases import bits, make_desc
from test_gpu_fuzz import sphere_soup, triangle_soup

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H, SPP, DEPTH = 64, 64, 2, 5
LDS, HBM_OCT, HBM_SHARED = 0, 1, 2


@pytest.fixture(scope="module")
def P():
    import path_tracer_ocaml_amd as P
    assert P.lib().ptx_device_count() >= 1, P.last_error()
    return P


@pytest.fixture(scope="module")
def driver():
    """tests/c/asan_host_driver.cpp as a plain program (no sanitizer: this module runs on the GPU machine)"""
    out = os.path.join(ROOT, "build", "lds_fit")
    os.makedirs(out, exist_ok=True)
    exe = os.path.join(out, "host_driver")
    host, csrc = os.path.join(ROOT, "path_tracer_ocaml_amd", "host"), os.path.join(ROOT, "path_tracer_ocaml_amd", "csrc")
    src = [os.path.join(ROOT, "tests", "c", "asan_host_driver.cpp")] + [os.path.join(host, f) for f in ("scenes.cpp", "png_write.cpp", "ply.cpp", "ppm_command.cpp")] + \
          [os.path.join(csrc, f) for f in ("bvh_build.cpp", "scene_host.cpp")]
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-march=x86-64-v3", "-ffp-contract=off", "-fno-fast-math", "-fno-math-errno", "-o", exe] + src)
    return exe


SOUPS = {  # name: (leaf kind, length cutoff, the largest soup tried)
    "simd_spheres": (0, 16, 6000),
    "array_spheres": (1, 4, 4000),
    "triangles": (1, 4, 2500),
}


def soup(name):
    rng = np.random.default_rng({"simd_spheres": 71, "array_spheres": 72, "triangles": 73}[name])
    centre, n = np.array([0.0, 0.0, -4.0]), SOUPS[name][2]
    return triangle_soup(rng, n, 1.5, centre, 2.0) if name == "triangles" else sphere_soup(rng, n, 1.5, centre, 2.0)


def desc(abi, name, prims, n):
    kind, cutoff, _ = SOUPS[name]
    return make_desc(abi, tris=prims[:n], leaf_kind=kind, cutoff=cutoff) if name == "triangles" else make_desc(abi, spheres=prims[:n], leaf_kind=kind, cutoff=cutoff)


def layout(P, driver, name, d, keep, **keys):
    """the header's answer for this scene: its integers from a host-only scene, the rest from `keys`"""
    host = P.Scene(d, -1, keepalive=keep)
    st = host.stats()
    host.close()
    kind = SOUPS[name][0]
    a = dict(mode=kind, n_nodes=st["tree_nodes"], total_slots=st["leaf_slots"], has_triangles=int(name == "triangles"), has_emit=0,
             tree_depth=st["tree_depth"], trace_waves=16 if kind == 0 else 8)
    a.update(keys)
    return json.loads(subprocess.check_output([driver, "layout", "ints"] + [f"{k}={v}" for k, v in a.items()]))


@pytest.fixture(scope="module")
def scenes(P, driver, oracle):
    """per soup: the largest LDS-resident prefix ("fits"), the next one ("beyond") and the largest that keeps the binary64 bounds in LDS
    ("fits64"), each with its descriptor and the oracle's render"""
    from path_tracer_ocaml_amd import abi
    memo = {}

    def get(name):
        if name not in memo:
            prims = soup(name)
            def last(pred):  # bisection: the largest prefix for which pred holds, and the next one, for which it does not
                lo, hi = 8, SOUPS[name][2]
                assert pred(lo) and not pred(hi), (name, "the boundary is not inside the sizes tried")
                while hi - lo > 1:
                    mid = (lo + hi) // 2
                    lo, hi = (mid, hi) if pred(mid) else (lo, mid)
                return lo, hi
            lo, hi = last(lambda n: layout(P, driver, name, *desc(abi, name, prims, n))["placement"] == LDS)
            lo64, _ = last(lambda n: layout(P, driver, name, *desc(abi, name, prims, n))["lds_nodes64_kept"] == 1)
            assert lo64 < lo
            memo[name] = {}
            for side, n in (("fits", lo), ("beyond", hi), ("fits64", lo64)):
                d, keep = desc(abi, name, prims, n)
                ref = oracle.Scene(C.pointer(d), keep).render(W, H, SPP, DEPTH, threads=8, want_raw=True, count=True)
                memo[name][side] = (n, d, keep, ref)
        return memo[name]
    return get


#          PTX_BOUNCE_THREADS, PTX_FUSED, PTX_BOUNCE_ORDER, PTX_LDS_NODES64
FITS = [(1024, 2, 0, 1),   # k_bounce: pools and parked walks behind the fullest image
        (1024, 2, 1, 1),   # k_bounce_carry: its parked entries there
        (64, 2, 0, 1),     # one wave: the smallest stacks, pools and park
        (64, 2, 1, 1),     # ... of k_bounce_carry
        (1024, 0, 0, 1)]   # k_trace + k_shade_pool on the LDS image
FITS64 = [(1024, 2, 0, 1),  # the binary64 bounds close the image: k_bounce,
          (1024, 2, 1, 1),  # k_bounce_carry,
          (1024, 0, 0, 1),  # k_trace + k_shade_pool;
          (1024, 2, 0, 0)]  # and the same scene without them
BEYOND = [(1024, 2, 0, 1),  # from HBM / L2: k_bounce on the per-octant image, or (the gap) the two kernels on the shared one
          (64, 2, 1, 1),    # ... asked for the shade-first order, which needs an LDS-resident scene
          (1024, 0, 0, 1)]  # k_trace + k_shade_pool


@pytest.mark.parametrize("side,threads,fused,order,nodes64", [("fits",) + c for c in FITS] + [("fits64",) + c for c in FITS64] + [("beyond",) + c for c in BEYOND])
@pytest.mark.parametrize("name", list(SOUPS))
def test_nearly_full_lds_renders_equal_the_oracle(P, driver, scenes, monkeypatch, name, side, threads, fused, order, nodes64):
    torch = pytest.importorskip("torch")
    n, d, keep, ref = scenes(name)[side]
    for k, v in (("PTX_BOUNCE_THREADS", threads), ("PTX_FUSED", fused), ("PTX_BOUNCE_ORDER", order), ("PTX_LDS_NODES64", nodes64)):
        monkeypatch.setenv(k, str(v))  # read when the scene handle is created
    lay = layout(P, driver, name, d, keep, waves=threads // 64)
    kept = int(bool(nodes64) and lay["lds_nodes64_kept"])
    lay = layout(P, driver, name, d, keep, waves=threads // 64, lds_nodes64=kept, hbm=int(lay["placement"] == HBM_OCT))
    assert (lay["placement"] == LDS) == (side != "beyond")
    if side != "beyond":  # the buffer is nearly full: one more primitive and the scene (fits64: the bounds) leaves LDS; and the carry record is never what gives first
        assert kept == int(side == "fits64" and nodes64 == 1)
        assert kept == 0 or lay["k_trace"]["nodes64"] < lay["k_trace"]["total"]
        assert lay["k_trace"]["total"] > 0.9 * 80 * 1024 or side == "fits64" and nodes64 == 0
        assert lay["k_bounce"]["fits"] and lay["k_bounce_carry"]["fits"]
    print(name, side, n, json.dumps(lay))
    g = P.Scene(d, 0, keepalive=keep)
    try:
        assert g.stats()["traversal_in_lds"] == (lay["placement"] == LDS)
        raw = torch.zeros((H, W, 3), dtype=torch.float64, device="cuda:0")
        st = g.render_raw_device(P.render_params(W, H, SPP, DEPTH, count_work=True, time_kernels=True), raw.data_ptr())
    finally:
        g.close()
    for k in ("segments", "nodes_tested", "prims_tested"):
        assert st[k] == ref["counters"][k], k
    assert np.array_equal(bits(raw.cpu().numpy()), bits(ref["raw"]))
    # what ran is what the layout said
    one_kernel = fused == 2 and (lay["k_bounce"]["fits"] if lay["placement"] == LDS else lay["placement"] == HBM_OCT)
    carry = one_kernel and order == 1 and lay["placement"] == LDS and lay["k_bounce_carry"]["fits"]
    launches = st["kernel_launches"]
    assert (st["carry_launches"] > 0) == carry
    if one_kernel:
        assert launches["bounce"] > 0 and launches["trace"] == 0 and launches["shade"] == 0
    else:  # the two-kernel fallback
        assert launches["bounce"] == 0 and launches["trace"] > 0 and launches["shade"] > 0
