"""ptx_intersect_rays against the exact, oracle-independent reference (tests/exact_geometry.py) on every walk the entry
point can take, the LDS top-of-tree walk (PTX_TRACE_TOP / PTX_TOP_NODES) against the oracle bit for bit, and the tree
invariants on GPU-built trees.  The switches are read when a scene is created, so they are set before P.Scene()."""
import ctypes as C

import numpy as np
import pytest

import exact_geometry as X

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def P():
    import path_tracer_ocaml_amd as P
    assert P.lib().ptx_device_count() >= 1, P.last_error()
    return P


@pytest.fixture(scope="module")
def refs(oracle):
    """name -> (ptr, keep, O, D, Result): one exact reference per scene, shared by every walk of that scene."""
    from path_tracer_ocaml_amd import abi
    cache = {}

    def get(name):
        if name not in cache:
            ptr, keep = X.scene_desc(name, oracle, abi)
            geo = X.Geometry(ptr)
            O, D = X.make_rays(geo, 2000 if name == "ganesha_150k" else 1500, seed=sum(map(ord, name)))
            cache[name] = (ptr, keep, geo, O, D, X.Reference(geo).closest(O, D))
        return cache[name]
    return get


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _force_builder(desc_ptr, which):
    from path_tracer_ocaml_amd import abi
    d = abi.SceneDesc()
    C.memmove(C.byref(d), desc_ptr, C.sizeof(d))
    d.reserved = which  # 1 host, 2 GPU
    return d


def _check_exact(P, name, refs, builder, expect_lds=None):
    ptr, keep, geo, O, D, res = refs(name)
    g = P.Scene(_force_builder(ptr, builder), 0, keepalive=keep)
    try:
        if expect_lds is not None:
            assert g.stats()["traversal_in_lds"] == expect_lds
        t, prim, _ = g.intersect_rays(O, D)
    finally:
        g.close()
    s = res.summary(t)
    print(f"\n{name} builder {builder}: {s}")
    bad = X.compare(res, prim, t)
    assert not bad, "\n".join(bad)
    floors = X.check_floors(name, s)
    assert not floors, "\n".join(floors)


LDS_SCENES = [n for n in X.SCENES if n != "ganesha_150k"]


@pytest.mark.parametrize("nodes64", [1, 0])
@pytest.mark.parametrize("builder", [1, 2])
@pytest.mark.parametrize("name", LDS_SCENES)
def test_lds_scene_closest_hits_equal_exact_reference(P, refs, name, builder, nodes64, monkeypatch):
    monkeypatch.setenv("PTX_LDS_NODES64", str(nodes64))
    _check_exact(P, name, refs, builder)


@pytest.mark.parametrize("env", [{}, {"PTX_OCT_IMAGE": "0"}, {"PTX_TRACE_TOP": "1", "PTX_TOP_NODES": "1"},
                                 {"PTX_TRACE_TOP": "1", "PTX_TOP_NODES": "64"}, {"PTX_TRACE_TOP": "1", "PTX_TOP_NODES": "1023"}],
                         ids=["octant_image", "no_octant_image", "top1", "top64", "top1023"])
@pytest.mark.parametrize("builder", [1, 2])
def test_hbm_mesh_closest_hits_equal_exact_reference(P, refs, builder, env, monkeypatch):
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    _check_exact(P, "ganesha_150k", refs, builder, expect_lds=False)


@pytest.mark.parametrize("top_nodes", [1, 64, 1023])
def test_trace_top_equals_oracle_bitwise(P, oracle, refs, top_nodes, monkeypatch):
    """The LDS top-of-tree walk of k_trace: hits, t bits and the work counters are the oracle's."""
    monkeypatch.setenv("PTX_TRACE_TOP", "1")
    monkeypatch.setenv("PTX_TOP_NODES", str(top_nodes))
    ptr, keep, geo, O, D, res = refs("ganesha_150k")
    g = P.Scene(ptr, 0, keepalive=keep)
    t_g, p_g, st = g.intersect_rays(O, D)
    g.close()
    t_c, p_c, ct = oracle.Scene(ptr, keep).intersect_rays(O, D)
    assert np.array_equal(p_g, p_c)
    assert np.array_equal(bits(t_g), bits(t_c))
    for k in ("nodes_tested", "prims_tested", "floor_tested"):
        assert st[k] == ct[k], k


def test_trace_top_render_equals_oracle_raw_sums(P, oracle, monkeypatch):
    """A small ganesha-like frame through k_trace + k_shade_pool with the top of the tree in LDS: raw sums bit for bit."""
    torch = pytest.importorskip("torch")
    w, h, spp, depth = 64, 40, 2, 5
    d = oracle.desc_ganesha_like(w, h, n_target=150000)
    c = oracle.Scene(d.ptr, d).render(w, h, spp, depth, threads=8, want_raw=True, count=True)
    monkeypatch.setenv("PTX_TRACE_TOP", "1")
    monkeypatch.setenv("PTX_FUSED_GLOBAL", "0")  # k_trace (the walk that reads the LDS top) rather than k_bounce
    g = P.Scene(d.ptr, 0, keepalive=d)
    assert not g.stats()["traversal_in_lds"]
    raw = torch.zeros((h, w, 3), dtype=torch.float64, device="cuda:0")
    st = g.render_raw_device(P.render_params(w, h, spp, depth, count_work=True), raw.data_ptr())
    g.close()
    for k in ("segments", "nodes_tested", "prims_tested"):
        assert st[k] == c["counters"][k], k
    assert np.array_equal(bits(raw.cpu().numpy()), bits(c["raw"]))


@pytest.mark.parametrize("name", ["shirley", "shirley_no_simd", "cornell", "ganesha_300", "ganesha_3k", "ganesha_9k",
                                  "ganesha_20k", "ganesha_60k", "ganesha_150k", "soup-mix-1-1-4", "soup-sph-0-16-4"])
def test_gpu_built_tree_invariants(P, oracle, name):
    """The invariants of tests/test_exact_geometry.py::test_host_built_tree_invariants on the GPU builder's trees, at sizes
    on both sides of its segment classes."""
    from path_tracer_ocaml_amd import abi
    sizes = {"ganesha_300": 300, "ganesha_9k": 9000, "ganesha_20k": 20000, "ganesha_60k": 60000}
    if name in sizes:
        od = oracle.desc_ganesha_like(64, 36, sizes[name])
        ptr, keep = od.ptr, od
    else:
        ptr, keep = X.scene_desc(name, oracle, abi)
    geo = X.Geometry(ptr)
    g = P.Scene(_force_builder(ptr, 2), 0, keepalive=keep)
    try:
        assert g.stats()["bvh_built_on_gpu"]
        bbox, info, order = g.tree()
    finally:
        g.close()
    msgs = X.check_tree(geo, bbox, info, order, P.lib().ptx_leaf_size())
    assert not msgs, "\n".join(msgs[:20])
