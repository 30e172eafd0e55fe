"""The per-octant LDS node image on the GPU (PTX_LDS_OCT, read when the scene handle is created): the non-counting
k_bounce_carry launches of a Simd_leaf scene whose launch buffer fits with it hold one 32-byte record per (direction octant, node)
and walk it with PtTraverser::walk_asm_oct; everything else keeps the shared image.  A ray's tests and their order are the same on
both, so raw per-pixel sums equal the CPU oracle's trace_samples sums bit for bit with PTX_LDS_OCT=0 and 1.
ptx_stats.lds_oct_launches says which image a render walked.

k_bounce_carry runs from depth 2 on (a batch of depth 1 is one k_bounce launch: tests/test_gpu_bounce_order.py), so a depth-1 render
walks the shared image whatever PTX_LDS_OCT says and its counter is 0.
"""
import numpy as np
import pytest

from test_gpu_edge_cases import both, make_desc
from test_gpu_fuzz import sphere_soup

pytestmark = pytest.mark.gpu


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


@pytest.fixture(scope="module")
def P():
    import path_tracer_ocaml_amd as P
    assert P.lib().ptx_device_count() >= 1, P.last_error()
    return P


def oracle_sums(o_scene, w, h, spp, depth):
    """Per-pixel sums of the oracle's per-sample radiance, added in pass order from zero as k_accum adds them."""
    ys, xs = np.mgrid[0:h, 0:w]
    raw = np.zeros((h, w, 3))
    for p in range(spp):
        c, _ = o_scene.trace_samples(w, h, spp, depth, xs.ravel(), ys.ravel(), np.full(w * h, p))
        raw = raw + np.asarray(c).reshape(h, w, 3)
    return raw


_REFS = {}


def shirley_ref(oracle, w, h, spp, depth, no_simd=False):
    key = (w, h, spp, depth, no_simd)
    if key not in _REFS:
        d = oracle.desc_shirley(w, h, no_simd=True) if no_simd else oracle.desc_shirley(w, h)
        _REFS[key] = (d, oracle_sums(oracle.Scene(d.ptr, d), w, h, spp, depth))
    return _REFS[key]


def render(P, torch, g, w, h, spp, depth, **kw):
    raw = torch.zeros((h, w, 3), dtype=torch.float64, device="cuda:0")
    st = g.render_raw_device(P.render_params(w, h, spp, depth, **kw), raw.data_ptr())
    return raw.cpu().numpy(), st


@pytest.mark.parametrize("no_simd", [False, True])
# (depth 1 runs NONE of the new code on either setting: a one-bounce batch is a single k_bounce launch, run_bounces takes k_bounce_carry
# from max_bounces = 2 on.  The case pins that such a render is exact and counts no launch on the per-octant image.)
@pytest.mark.parametrize("w,h,depth", [(64, 40, 8), (64, 40, 1), (13, 9, 8)])
def test_shirley_both_images(P, oracle, w, h, depth, no_simd, monkeypatch):
    """13 x 9: ragged tiles and lanes without a sample in the camera launch.  no_simd (Array_leaf) keeps the shared image."""
    torch = pytest.importorskip("torch")
    spp = 2
    d, want = shirley_ref(oracle, w, h, spp, depth, no_simd)
    for oct_ in ("0", "1"):
        monkeypatch.setenv("PTX_LDS_OCT", oct_)
        g = P.Scene(d.ptr, 0, keepalive=d)
        assert g.stats()["traversal_in_lds"] == 1
        got, st = render(P, torch, g, w, h, spp, depth)
        assert np.array_equal(bits(got), bits(want)), (oct_, "not counting")
        ran = oct_ == "1" and not no_simd and depth >= 2
        assert (st["lds_oct_launches"] > 0) == ran, (oct_, st["lds_oct_launches"])
        got, st = render(P, torch, g, w, h, spp, depth, count_work=True)  # counting renders keep the shared image and loop
        assert np.array_equal(bits(got), bits(want)), (oct_, "counting")
        assert st["lds_oct_launches"] == 0
        g.close()


@pytest.mark.parametrize("fence_wg", ["0", "1"])
@pytest.mark.parametrize("streams", ["1", "2"])
def test_fences_and_streams(P, oracle, fence_wg, streams, monkeypatch):
    torch = pytest.importorskip("torch")
    w, h, spp, depth = 64, 40, 2, 8
    d, want = shirley_ref(oracle, w, h, spp, depth)
    monkeypatch.setenv("PTX_BOUNCE_FENCE_WG", fence_wg)
    monkeypatch.setenv("PTX_STREAMS", streams)
    for oct_ in ("0", "1"):
        monkeypatch.setenv("PTX_LDS_OCT", oct_)
        g = P.Scene(d.ptr, 0, keepalive=d)
        got, st = render(P, torch, g, w, h, spp, depth, passes_per_batch=1)  # two batches: both streams carry one
        assert np.array_equal(bits(got), bits(want)), oct_
        assert (st["lds_oct_launches"] > 0) == (oct_ == "1")
        g.close()


# ---- sphere soups: the admit decision, restated from the layout's description (csrc/pt_lds_layout.h) ----
LIMIT = 160 * 1024 - (2 * 256 * 4 + 512)
WAVES = 16


def shared_end(n, slots, depth, n64):
    stacks = (WAVES * (depth + 1) * 16 + 63) & ~63
    return stacks + ((n * 92 + 63) & ~63) + slots * 32 + ((slots + 15) & ~15) + (48 * n if n64 else 0)


def keeps_nodes64(n, slots, depth):
    """pt_lds_keep_nodes64: LDS-resident at k_trace's workgroup size without and with the binary64 bounds, and k_bounce fits with them"""
    if 2048 + WAVES * (depth + 1) * 16 + n * 92 >= 65534:
        return None  # not LDS-resident at all
    if shared_end(n, slots, depth, 0) > 80 * 1024:
        return None
    if shared_end(n, slots, depth, 1) > 80 * 1024:
        return 0
    pool = (shared_end(n, slots, depth, 1) + 63) & ~63
    return int(pool + WAVES * 5 * 128 * 6 + (64 + WAVES * 16) * 16 <= LIMIT)


def oct_fits(n, slots, n64):
    end = 256 * n + 4 * ((n + 3) & ~3) + 32 * slots + ((slots + 15) & ~15) + (48 * n if n64 else 0)
    return ((end + 63) & ~63) + 6 * (64 + WAVES * 16) * 16 <= LIMIT


def soup_desc(n, seed=11, scale=1.0):
    from path_tracer_ocaml_amd import abi
    rng = np.random.default_rng(seed)
    centre = np.array([0.2, -0.1, -5.0]) * scale
    return make_desc(abi, spheres=sphere_soup(rng, n, scale, centre, 2.0), leaf_kind=0, cutoff=16)


def soup_scene(P, oracle, n, seed=11, scale=1.0):
    return both(P, oracle, *soup_desc(n, seed, scale))


def check_soup(P, torch, o_scene, g_scene, expect_oct):
    w, h, spp, depth = 32, 32, 2, 4
    want = oracle_sums(o_scene, w, h, spp, depth)
    got, st = render(P, torch, g_scene, w, h, spp, depth)
    assert np.array_equal(bits(got), bits(want))
    assert (st["lds_oct_launches"] > 0) == expect_oct, st["lds_oct_launches"]
    return st


@pytest.mark.parametrize("n", [1, 2, 17])
def test_small_soups(P, oracle, n, monkeypatch):
    torch = pytest.importorskip("torch")
    monkeypatch.setenv("PTX_BOUNCE_ORDER", "1")  # a soup is not binned by elevation: ask for the shade-first order
    for oct_ in ("0", "1"):
        monkeypatch.setenv("PTX_LDS_OCT", oct_)
        o_scene, g_scene = soup_scene(P, oracle, n)
        check_soup(P, torch, o_scene, g_scene, oct_ == "1")
        g_scene.close()


def test_soups_at_the_capacity_bound(P, oracle, monkeypatch):
    """The largest soup of a family whose launch buffer still fits with the per-octant image walks it; the next one of the family
    that does not fit keeps the shared image.  Both bit-exact."""
    torch = pytest.importorskip("torch")
    monkeypatch.setenv("PTX_BOUNCE_ORDER", "1")
    monkeypatch.setenv("PTX_LDS_OCT", "1")
    under = over = None  # (sphere count, tree nodes)
    for n in range(420, 900, 6):
        d, keep = soup_desc(n)
        g_scene = P.Scene(d, 0, keepalive=keep)
        st = g_scene.stats()
        g_scene.close()
        n64 = keeps_nodes64(st["tree_nodes"], st["leaf_slots"], st["tree_depth"])
        assert n64 is not None and st["traversal_in_lds"] == 1
        if not oct_fits(st["tree_nodes"], st["leaf_slots"], n64):
            over = (n, st["tree_nodes"])
            break
        under = (n, st["tree_nodes"])
    assert under is not None and over is not None, "the family did not cross the bound"
    assert 0 < over[1] - under[1] < 24, (under, over)  # a few nodes apart
    for (n, _), ran in ((under, True), (over, False)):
        o_scene, g_scene = soup_scene(P, oracle, n)
        check_soup(P, torch, o_scene, g_scene, ran)
        g_scene.close()


def test_every_ray_in_binary64(P, oracle, monkeypatch):
    """Coordinates beyond binary32 (the fuzz module's 1e39 scaling): the filter's guard sends every test of every ray to binary64, so
    every visit of the assembly loop leaves through its undecided exit and the C++ visit finds its binary64 node from a record number."""
    torch = pytest.importorskip("torch")
    monkeypatch.setenv("PTX_BOUNCE_ORDER", "1")
    w, h, spp, depth = 32, 32, 2, 4
    for oct_ in ("0", "1"):
        monkeypatch.setenv("PTX_LDS_OCT", oct_)
        o_scene, g_scene = soup_scene(P, oracle, 120, seed=77, scale=1e39)
        with np.errstate(over="ignore", invalid="ignore"):
            want = oracle_sums(o_scene, w, h, spp, depth)
        got, st = render(P, torch, g_scene, w, h, spp, depth, count_work=True)
        assert st["filter_undecided"] > 0 and st["lds_oct_launches"] == 0
        assert st["segments"] > w * h * spp  # some camera ray hits the soup and goes on
        assert np.array_equal(bits(got), bits(want))
        got, st = render(P, torch, g_scene, w, h, spp, depth)
        assert np.array_equal(bits(got), bits(want)), oct_
        assert (st["lds_oct_launches"] > 0) == (oct_ == "1")
        g_scene.close()
