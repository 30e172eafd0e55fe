"""Camera tile lists on the GPU (PTX_TILE_LISTS, read when the scene handle is created): the non-counting camera
launch of k_bounce_carry on the per-octant LDS image scans, per 8 x 8 tile, the list of spheres a camera ray of the tile can meet
instead of walking the tree; tiles marked "walk", chunks with a ray of another octant and chunks in which a guard of the scan fires
walk as before.  A ray's hit is the walk's, so raw per-pixel sums equal the CPU oracle's and PTX_TILE_LISTS=0's bit for bit.
ptx_tile_list_stats says what the last render did; counting renders keep the walk and the oracle's work counters.

k_bounce_carry runs from depth 2 on (tests/test_gpu_lds_oct.py), so a depth-1 render scans nothing whatever the knob says.
"""
import ctypes as C

import numpy as np
import pytest

from test_gpu_edge_cases import make_desc
from test_tile_lists import soup, special_soups, stacked

pytestmark = pytest.mark.gpu

COUNTERS = ("segments", "nodes_tested", "prims_tested", "floor_tested")
SPP = 3


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


@pytest.fixture(scope="module")
def P():
    import path_tracer_ocaml_amd as P
    assert P.lib().ptx_device_count() >= 1, P.last_error()
    return P


_REFS = {}


def shirley_ref(oracle, w, h, depth):
    if (w, h, depth) not in _REFS:
        d = oracle.desc_shirley(w, h)
        _REFS[w, h, depth] = (d, oracle.Scene(d.ptr, d).render(w, h, SPP, depth, threads=8, want_raw=True, count=True))
    return _REFS[w, h, depth]


def render(P, torch, g, w, h, depth, **kw):
    raw = torch.zeros((h, w, 3), dtype=torch.float64, device="cuda:0")
    st = g.render_raw_device(P.render_params(w, h, SPP, depth, **kw), raw.data_ptr())
    return raw.cpu().numpy(), st, g.tile_list_stats()


def walk_tiles_by_sign(w, h):
    """tiles whose direction bounds straddle or touch zero under make_desc's camera (-1, -0.5, 2, 1): the columns around w / 2, the rows around h / 2"""
    tx, ty = (w + 7) // 8, (h + 7) // 8
    cols = sum(1 for t in range(tx) if 8 * t <= w / 2 <= min(8 * t + 8, w))
    rows = sum(1 for t in range(ty) if 8 * t <= h / 2 <= min(8 * t + 8, h))
    return cols * ty + rows * tx - cols * rows


@pytest.mark.parametrize("streams", ["1", "2"])
@pytest.mark.parametrize("depth", [8, 1])
def test_shirley_ragged_tiles(P, oracle, depth, streams, monkeypatch):
    """61 x 37: ragged tiles in both axes, and the tile row across the horizon, whose rays have both signs of d.y, keeps the walk."""
    torch = pytest.importorskip("torch")
    w, h = 61, 37
    d, want = shirley_ref(oracle, w, h, depth)
    monkeypatch.setenv("PTX_STREAMS", streams)
    for knob in ("0", "1"):
        monkeypatch.setenv("PTX_TILE_LISTS", knob)
        g = P.Scene(d.ptr, 0, keepalive=d)
        got, st, tl = render(P, torch, g, w, h, depth, passes_per_batch=2)  # two batches: with two streams each carries one
        assert np.array_equal(bits(got), bits(want["raw"])), (knob, "not counting")
        if knob == "1" and depth >= 2:
            assert tl["list_launches"] == 2 and tl["tiles"] == 8 * 5 and 0 < tl["walk_tiles"] < 40 and 0 < tl["longest_list"] <= 15, tl
        else:
            assert not any(tl.values()), tl
        got, st, tl = render(P, torch, g, w, h, depth, passes_per_batch=2, count_work=True)  # counting renders keep the walk
        assert np.array_equal(bits(got), bits(want["raw"])), (knob, "counting")
        assert not any(tl.values()), tl
        for k in COUNTERS:
            assert st[k] == want["counters"][k], (knob, k)
        g.close()


def soup_both(P, oracle, spheres):
    from path_tracer_ocaml_amd import abi
    d, keep = make_desc(abi, spheres=[(*s, i % 3) for i, s in enumerate(spheres)], leaf_kind=0, cutoff=16)
    return oracle.Scene(C.pointer(d), keep), P.Scene(d, 0, keepalive=keep)


def check_soup(P, oracle, torch, monkeypatch, spheres, w=64, h=40, depth=4):
    """Both settings of the knob against the oracle; returns the stats of the render that scanned"""
    monkeypatch.setenv("PTX_BOUNCE_ORDER", "1")  # a soup is not binned by elevation: ask for the shade-first order
    out = None
    for knob in ("0", "1"):
        monkeypatch.setenv("PTX_TILE_LISTS", knob)
        o_scene, g = soup_both(P, oracle, spheres)
        want = o_scene.render(w, h, SPP, depth, threads=8, want_raw=True)["raw"]
        got, st, tl = render(P, torch, g, w, h, depth)
        assert np.array_equal(bits(got), bits(want)), knob
        assert st["lds_oct_launches"] > 0
        assert (tl["list_launches"] > 0) == (knob == "1"), tl
        out = tl
        g.close()
    return out


@pytest.mark.parametrize("n", [1, 2, 17])
def test_small_soups(P, oracle, n, monkeypatch):
    torch = pytest.importorskip("torch")
    tl = check_soup(P, oracle, torch, monkeypatch, soup(n))
    assert tl["tiles"] == 40 and tl["walk_tiles"] == walk_tiles_by_sign(64, 40)


def test_overflow_tile_walks(P, oracle, monkeypatch):
    """40 spheres behind one tile: more candidates than a record holds"""
    torch = pytest.importorskip("torch")
    tl = check_soup(P, oracle, torch, monkeypatch, stacked(40))
    assert tl["walk_tiles"] > walk_tiles_by_sign(64, 40) and tl["longest_list"] <= 15


def test_guards_send_chunks_back(P, oracle, monkeypatch):
    """Two coincident spheres tie on every ray that hits them, two tangent ones where they meet: the tie guard fires and those chunks walk"""
    torch = pytest.importorskip("torch")
    tl = check_soup(P, oracle, torch, monkeypatch, special_soups()["coincident_tangent"][0])
    assert tl["fallback_chunks"] > 0, tl


def test_band_shard(P, oracle, monkeypatch):
    """Rank 1 of 3 with bands of 8 rows: the global grid indexed through pt_global_row"""
    torch = pytest.importorskip("torch")
    w, h, depth = 61, 37, 8
    d, want = shirley_ref(oracle, w, h, depth)
    pr = P.render_params(w, h, SPP, depth, band_rows=8, band_first=1, band_step=3)
    rows = P.local_rows(pr)
    gy = [P.global_row(pr, k) for k in range(rows)]
    assert 0 < rows < h
    for knob in ("0", "1"):
        monkeypatch.setenv("PTX_TILE_LISTS", knob)
        g = P.Scene(d.ptr, 0, keepalive=d)
        part = torch.zeros((rows, w, 3), dtype=torch.float64, device="cuda:0")
        g.render_raw_device(pr, part.data_ptr())
        tl = g.tile_list_stats()
        assert np.array_equal(bits(part.cpu().numpy()), bits(want["raw"][gy])), knob
        assert (tl["list_launches"] > 0) == (knob == "1") and tl["tiles"] == (40 if knob == "1" else 0), tl
        g.close()


def test_two_image_sizes_on_one_scene(P, oracle, monkeypatch):
    """The grid belongs to (scene, image size): built at the first render of a size, found again at the next.  Shirley's tree and camera
    height do not depend on the image size, only the camera's width does: one handle per aspect ratio, two sizes of it in turn."""
    torch = pytest.importorskip("torch")
    monkeypatch.setenv("PTX_TILE_LISTS", "1")
    depth = 8
    d, want_a = shirley_ref(oracle, 61, 37, depth)
    g = P.Scene(d.ptr, 0, keepalive=d)
    o_scene = oracle.Scene(d.ptr, d)
    want_b = o_scene.render(122, 74, SPP, depth, threads=8, want_raw=True)["raw"]  # the same aspect ratio: the same camera
    for w, h, want, tiles in ((61, 37, want_a["raw"], 40), (122, 74, want_b, 16 * 10), (61, 37, want_a["raw"], 40), (122, 74, want_b, 160)):
        got, st, tl = render(P, torch, g, w, h, depth)
        assert np.array_equal(bits(got), bits(want)), (w, h)
        assert tl["list_launches"] > 0 and tl["tiles"] == tiles, tl
    g.close()
