"""The camera launch of k_bounce_carry hands shade 0 its sample, its ray and its hit in registers (PtCameraCarry, csrc/kernels.hip;
DESIGN.md section 4): the lane that generated and walked a camera ray shades it, category step by category step, on the decoded sample
(path id, sampler offset), the direction and the hit distance it still holds, instead of storing the distance, fencing, and decoding,
deriving and loading all three again in every step.  The values are the same, so raw per-pixel sums equal the CPU oracle's bit for bit on
every camera instantiation: packet walk and lane walk, shared and per-octant image, scanned and walked tiles, counting and not, with and
without emitters -- and on triangle scenes, where the distance is recomputed and only the sample and the direction are carried.

k_bounce_carry runs from depth 2 on (tests/test_gpu_lds_oct.py); depth 2 is the camera launch plus the shade-only launch.
The shapes are the smallest at which the branch can go wrong: ragged tiles in both axes (lanes of a live chunk without a sample), a
ragged last batch, several categories in one 8 x 8 tile (every lane must get its own ray in its own step), and tiles nothing hits.
"""
import ctypes as C
import itertools

import numpy as np
import pytest

from test_gpu_edge_cases import make_desc
from test_gpu_fuzz import sphere_soup
from test_tile_lists import soup

pytestmark = pytest.mark.gpu

COUNTERS = ("segments", "nodes_tested", "prims_tested", "floor_tested")
SPP, PPB = 3, 2
N_BATCHES = (SPP + PPB - 1) // PPB


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


@pytest.fixture(scope="module")
def P():
    import path_tracer_ocaml_amd as P
    assert P.lib().ptx_device_count() >= 1, P.last_error()
    return P


_REFS = {}


def ref(oracle, kind, w, h, spp, depth):
    """The oracle's counting render of a stock scene, computed once and shared."""
    key = (kind, w, h, spp, depth)
    if key not in _REFS:
        d = {"shirley": oracle.desc_shirley, "cornell": oracle.desc_cornell}[kind](w, h)
        _REFS[key] = (d, oracle.Scene(d.ptr, d).render(w, h, spp, depth, threads=8, want_raw=True, count=True))
    return _REFS[key]


def render(P, torch, g, w, h, spp, depth, **kw):
    raw = torch.zeros((h, w, 3), dtype=torch.float64, device="cuda:0")
    st = g.render_raw_device(P.render_params(w, h, spp, depth, **kw), raw.data_ptr())
    return raw.cpu().numpy(), st


def check_counting(st, want, where):
    for k in COUNTERS:
        assert st[k] == want["counters"][k], (where, k, st[k], want["counters"][k])
    assert st["carry_launches"] > 0, where  # the shade-first order ran


@pytest.mark.parametrize("fence_wg", ["0", "1"])
@pytest.mark.parametrize("streams", ["1", "2"])
@pytest.mark.parametrize("depth", [8, 2])
def test_shirley_every_camera_instantiation(P, oracle, depth, streams, fence_wg, monkeypatch):
    """61 x 37, spp 3 in batches of 2: tile lists x per-octant image x walk, not counting and counting (the counting renders keep the
    shared image, the C++ loop and the walk, and must count what the oracle counts)."""
    torch = pytest.importorskip("torch")
    w, h = 61, 37
    d, want = ref(oracle, "shirley", w, h, SPP, depth)
    monkeypatch.setenv("PTX_STREAMS", streams)
    monkeypatch.setenv("PTX_BOUNCE_FENCE_WG", fence_wg)
    seen = set()
    for tile, oct_, walk in itertools.product("01", "01", "01"):
        monkeypatch.setenv("PTX_TILE_LISTS", tile)
        monkeypatch.setenv("PTX_LDS_OCT", oct_)
        monkeypatch.setenv("PTX_PRIMARY_WALK", walk)
        where = (tile, oct_, walk)
        g = P.Scene(d.ptr, 0, keepalive=d)
        got, st = render(P, torch, g, w, h, SPP, depth, passes_per_batch=PPB)
        assert np.array_equal(bits(got), bits(want["raw"])), (where, "not counting")
        tl = g.tile_list_stats()
        seen.add((st["lds_oct_launches"] > 0, tl["list_launches"] > 0))
        got, st = render(P, torch, g, w, h, SPP, depth, passes_per_batch=PPB, count_work=True)
        assert np.array_equal(bits(got), bits(want["raw"])), (where, "counting")
        check_counting(st, want, where)
        assert st["primary_lane_walks"] == (N_BATCHES if walk == "1" else 0), where
        g.close()
    # the shared image, the per-octant image walked, and the per-octant image with scanned tiles all ran
    assert seen == {(False, False), (True, False), (True, True)}, seen


def soup_both(P, oracle, spheres):
    from path_tracer_ocaml_amd import abi
    d, keep = make_desc(abi, spheres=[(*s, i % 3) for i, s in enumerate(spheres)], leaf_kind=0, cutoff=16)
    return oracle.Scene(C.pointer(d), keep), P.Scene(d, 0, keepalive=keep)


def tile_categories(o_scene, w, h):
    """Per 8 x 8 tile, the set of what the pixel centres' camera rays meet under make_desc's camera (-1, -0.5, 2, 1): -1 for a miss,
    else the material i % 3 of primitive i"""
    ys, xs = np.mgrid[0:h, 0:w]
    cx, cy = (xs.ravel() + 0.5) / w, 1.0 - (ys.ravel() + 0.5) / h
    dirs = np.stack([-1.0 + 2.0 * cx, -0.5 + 1.0 * cy, -np.ones(w * h)], axis=1)
    dirs /= np.linalg.norm(dirs, axis=1, keepdims=True)
    _, prim, _ = o_scene.intersect_rays(np.zeros((w * h, 3)), dirs)
    cat = np.where(prim < 0, -1, prim % 3).reshape(h, w)
    return [set(cat[ty:ty + 8, tx:tx + 8].ravel().tolist()) for ty in range(0, h, 8) for tx in range(0, w, 8)]


def check_soup(P, oracle, torch, monkeypatch, spheres, w=64, h=40, depth=4):
    """Scanned and walked tiles, lane walk and packet walk, against the oracle; returns the oracle scene's per-tile categories"""
    monkeypatch.setenv("PTX_BOUNCE_ORDER", "1")  # a soup is not binned by elevation: ask for the shade-first order
    cats = want = None
    for tile, walk in itertools.product("01", "01"):
        monkeypatch.setenv("PTX_TILE_LISTS", tile)
        monkeypatch.setenv("PTX_PRIMARY_WALK", walk)
        o_scene, g = soup_both(P, oracle, spheres)
        if want is None:
            want = o_scene.render(w, h, SPP, depth, threads=8, want_raw=True, count=True)
            cats = tile_categories(o_scene, w, h)
        got, st = render(P, torch, g, w, h, SPP, depth)
        assert np.array_equal(bits(got), bits(want["raw"])), (tile, walk)
        assert (st["lds_oct_launches"] > 0) == (walk == "1"), (tile, walk)  # (the per-octant image: camera rays one per lane)
        assert (g.tile_list_stats()["list_launches"] > 0) == (tile == "1" and walk == "1"), (tile, walk)
        got, st = render(P, torch, g, w, h, SPP, depth, count_work=True)
        assert np.array_equal(bits(got), bits(want["raw"])), (tile, walk, "counting")
        check_counting(st, want, (tile, walk))
        g.close()
    return cats, want


@pytest.mark.parametrize("n", [1, 2, 17])
def test_soups_with_several_categories_in_a_tile(P, oracle, n, monkeypatch):
    torch = pytest.importorskip("torch")
    cats, want = check_soup(P, oracle, torch, monkeypatch, soup(n))
    assert want["counters"]["segments"] > 64 * 40 * SPP  # some camera sample hits and goes on: a chunk with a hit lane among misses
    if n == 17:
        # (pixel centres on the oracle) tiles in which two materials meet besides the sky: three category steps on one chunk
        assert any(len(c - {-1}) >= 2 for c in cats) and max(len(c) for c in cats) >= 3, sorted(map(len, cats))


def test_soup_every_camera_ray_misses(P, oracle, monkeypatch):
    """Spheres behind the camera: only the MISS step runs, nothing survives the camera launch, the later launches find empty queues"""
    torch = pytest.importorskip("torch")
    rng = np.random.default_rng(5)
    behind = np.array([s[:4] for s in sphere_soup(rng, 6, 1.0, np.array([0.3, 0.2, 5.0]), 1.0)])
    cats, want = check_soup(P, oracle, torch, monkeypatch, behind)
    assert all(c == {-1} for c in cats)
    assert want["counters"]["segments"] == 64 * 40 * SPP  # every path is its camera ray


@pytest.mark.parametrize("walk", ["0", "1"])
def test_cornell_emitters_and_recomputed_distance(P, oracle, walk, monkeypatch):
    """A closed box of triangles and spheres under an emissive ceiling, 32 x 24: the EMIT instantiations; with triangles in the scene
    the shade step recomputes t from the carried direction and the primitive."""
    torch = pytest.importorskip("torch")
    w, h, depth = 32, 24, 4
    d, want = ref(oracle, "cornell", w, h, SPP, depth)
    monkeypatch.setenv("PTX_BOUNCE_ORDER", "1")
    monkeypatch.setenv("PTX_PRIMARY_WALK", walk)
    g = P.Scene(d.ptr, 0, keepalive=d)
    assert g.stats()["traversal_in_lds"] == 1
    for streams in ("1", "2"):
        monkeypatch.setenv("PTX_STREAMS", streams)
        got, st = render(P, torch, g, w, h, SPP, depth, passes_per_batch=PPB)
        assert np.array_equal(bits(got), bits(want["raw"])), (streams, "not counting")
        got, st = render(P, torch, g, w, h, SPP, depth, passes_per_batch=PPB, count_work=True)
        assert np.array_equal(bits(got), bits(want["raw"])), (streams, "counting")
        check_counting(st, want, streams)
        assert st["primary_lane_walks"] == (N_BATCHES if walk == "1" else 0)
    g.close()


@pytest.mark.parametrize("w,h,spp,ppb", [(13, 9, 5, 3), (75, 43, 5, 3), (75, 43, 7, 4)])
def test_ragged_last_batch_and_ragged_tiles(P, oracle, w, h, spp, ppb, monkeypatch):
    """The last batch holds fewer passes than the others (5 = 3 + 2, 7 = 4 + 3) and the tile count (2 x 2, 10 x 6) times its passes is
    no multiple of the runs of chunks the workgroups are dealt; 13 x 9 and 75 x 43 leave lanes without a sample in the last tile
    column and row of every pass.  One wave takes every chunk, then the default grid."""
    torch = pytest.importorskip("torch")
    depth = 8
    d, want = ref(oracle, "shirley", w, h, spp, depth)
    for threads, wgs in ((64, 1), (0, 0)):
        monkeypatch.setenv("PTX_BOUNCE_THREADS", str(threads))
        monkeypatch.setenv("PTX_BOUNCE_WGS", str(wgs))
        for tile in ("0", "1"):
            monkeypatch.setenv("PTX_TILE_LISTS", tile)
            g = P.Scene(d.ptr, 0, keepalive=d)
            got, st = render(P, torch, g, w, h, spp, depth, passes_per_batch=ppb)
            assert np.array_equal(bits(got), bits(want["raw"])), (threads, tile, "not counting")
            got, st = render(P, torch, g, w, h, spp, depth, passes_per_batch=ppb, count_work=True)
            assert np.array_equal(bits(got), bits(want["raw"])), (threads, tile, "counting")
            check_counting(st, want, (threads, tile))
            g.close()
