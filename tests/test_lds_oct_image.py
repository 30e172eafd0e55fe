"""The per-octant LDS node image (PtHostArrays.lds_oct, csrc/scene_host.cpp) and its place in a k_bounce_carry launch's LDS buffer
(pt_lds_oct_layout, csrc/pt_lds_layout.h), without a GPU: build/asan/lds_oct_driver assembles scenes with the code the library ships,
under AddressSanitizer + UndefinedBehaviorSanitizer, and dumps what it made.

* Every record's six bounds are the sign-selected bounds of the node, rounded to binary32 as the shared LDS image rounds them
  (nodes32 holds exactly those roundings), and word 7 is the magnitude word pt_scene_view stores in the shared image.
* Every hit / miss link and every leaf-table entry is checked against a near-child-first descent of the tree for all eight octants,
  with test_scene_host's check_walk.
* The layout's offsets and its admit / refuse decision at the edges, and the headline tree's total.
"""
import json
import os

import numpy as np
import pytest

from test_sanitizers import ENV, ROOT, built, run_clean  # noqa: F401  (built: the `make asan` fixture)
from test_scene_host import END, NODE, check_walk

LEAF_TAG, OCT_END, MAX_NODES = 0x4000, 0x8000, 2047
LIMIT = 160 * 1024 - (2 * 256 * 4 + 512)  # PT_LDS_BOUNCE_LIMIT
PARK = (64 + 16 * 16) * 16  # PT_PARK_CAP(16 waves, cut 16) 16-byte words, per field


def image(built, scene, tmp_path, *opts):
    out = run_clean([os.path.join(built, "lds_oct_driver"), "image", scene, str(tmp_path), *opts])
    f = out.split()
    info = {f[i]: int(f[i + 1]) for i in range(0, len(f), 2)}
    nodes = np.fromfile(os.path.join(tmp_path, "nodes.bin"), dtype=NODE)
    nodes32 = np.fromfile(os.path.join(tmp_path, "nodes32.bin"), dtype="<u4").reshape(-1, 8)
    img = np.fromfile(os.path.join(tmp_path, "lds_oct.bin"), dtype="<u4")
    return info, nodes, nodes32, img


def layout(built, **kv):
    return json.loads(run_clean([os.path.join(built, "lds_oct_driver"), "layout"] + [f"{k}={v}" for k, v in kv.items()]))


@pytest.mark.parametrize("scene,n_expect", [("shirley", 341), ("soup17", None), ("soup300", None), ("soup1", 1)])
def test_records_links_and_leaf_table(built, tmp_path, scene, n_expect):
    info, nodes, nodes32, img = image(built, scene, tmp_path)
    n = len(nodes)
    assert n == info["nodes"] and (n_expect is None or n == n_expect)
    leaf_words = (n + 3) & ~3
    assert len(img) == info["words"] == 64 * n + leaf_words
    rec, table = img[: 64 * n].reshape(8, n, 8), img[64 * n:]
    leaf = (nodes["b"] >> 30) == 3
    assert leaf.any() and (scene == "soup1" or (~leaf).any())
    # the binary32 roundings of the bounds (what pt_scene_view stores in the shared image: (float)mn, (float)mx)
    lo, hi = nodes["mn"].astype(np.float32), nodes["mx"].astype(np.float32)
    assert np.array_equal(nodes32[:, 0:3].view(np.float32), lo) and np.array_equal(nodes32[:, 3:6].view(np.float32), hi)
    # word 7 of the shared image: max |bound| * 1.000001f, rounded up to a multiple of 4 in its bits, the axis in the two low bits
    mag = np.maximum(np.abs(lo), np.abs(hi)).max(axis=1).astype(np.float32) * np.float32(1.000001)
    word7 = ((mag.view(np.uint32) + np.uint32(4)) & np.uint32(0xFFFFFFFC)) | (nodes["b"] >> 30)
    for o in range(8):
        for a in range(3):
            pos = (o >> a) & 1  # component a of the direction >= 0: near = mn
            near, far = (lo, hi) if pos else (hi, lo)
            assert np.array_equal(rec[o, :, a].view(np.float32).view(np.uint32), near[:, a].view(np.uint32)), (o, a)
            assert np.array_equal(rec[o, :, 3 + a].view(np.float32).view(np.uint32), far[:, a].view(np.uint32)), (o, a)
        assert np.array_equal(rec[o, :, 7], word7), o
        base = o * n

        def node_of(ref):
            if ref == OCT_END:
                return END
            assert base <= (ref & (LEAF_TAG - 1)) < base + n and ref < OCT_END  # links carry the octant's base, 14 bits
            return (ref & (LEAF_TAG - 1)) - base

        def visit(ref):
            assert not ref & LEAF_TAG  # the walk visits plain record numbers
            k = ref - base
            hit, miss = int(rec[o, k, 6]) & 0xFFFF, int(rec[o, k, 6]) >> 16
            if leaf[k]:  # a hit holds the leaf (its own record under the tag); afterwards the walk goes on at the miss link
                assert hit == (LEAF_TAG | ref)
                assert int(table[k]) == int(nodes["a"][k]) | (int(nodes["pad"][k, 0]) << 16)
                return k, miss, miss
            assert not hit & (LEAF_TAG | OCT_END)
            return k, hit, miss
        check_walk(nodes, o, base, visit, node_of)
    assert not table[:n][~leaf].any() and not table[n:].any()


def test_switched_off_and_too_large(built, tmp_path):
    info, nodes, _, img = image(built, "shirley", tmp_path, "lds_oct=0")
    assert len(img) == 0 and len(nodes) == 341
    info, nodes, _, img = image(built, "soup20000", tmp_path)  # more than 2047 nodes: record numbers would not fit 14 bits
    assert len(nodes) > MAX_NODES and len(img) == 0
    # fewer than 2048 nodes, but records + leaf table + spheres alone are beyond what a launch may ask for: never admitted, not built
    info, nodes, _, img = image(built, "soup1500", tmp_path)
    n, slots = len(nodes), info["slots"]
    assert n <= MAX_NODES and expected(n, slots, 0)["end"] > LIMIT and len(img) == 0
    info, nodes, _, img = image(built, "soup700", tmp_path)  # beyond a launch WITH its parked entries, but not without: built, refused later
    n, slots = len(nodes), info["slots"]
    assert expected(n, slots, 0)["end"] <= LIMIT < expected(n, slots, 0)["total"] and len(img) == 64 * n + ((n + 3) & ~3)


def expected(n, slots, n64, emit=0):
    """The layout from its description: records | leaf table (to 16) | spheres | categories (to 16) | binary64 bounds; parked entries
    (6 words of 16 bytes per entry, 8 with emission) from the next multiple of 64."""
    leaf = 256 * n
    sph = leaf + 4 * ((n + 3) & ~3)
    cat = sph + 32 * slots
    nodes64 = cat + ((slots + 15) & ~15)
    end = nodes64 + (48 * n if n64 else 0)
    pool = (end + 63) & ~63
    return {"oct": 0, "leaf": leaf, "sph": sph, "cat": cat, "nodes64": nodes64, "end": end, "pool_off": pool, "park0": pool,
            "park_emit": pool + 6 * PARK, "park_end": pool + (8 if emit else 6) * PARK, "total": pool + (8 if emit else 6) * PARK}


def test_headline_total(built):
    """Shirley's tree, 341 nodes, 684 slots, depth 10.  With the shared image the launch's buffer is 103 936 bytes: stacks 2816 + nodes
    31 424 + spheres 21 888 + categories 688 + binary64 bounds 16 368 (+ 32 to the next multiple of 64) + parked entries 30 720.  With
    341 x 256 = 87 296 bytes of records in place of the 31 424 that is 159 808.  The layout as built differs from that figure by
    exactly three terms: it lays out no stacks (- 2816), it holds the leaf table (+ 344 x 4 = 1376), and its image ends on a
    multiple of 64 (- 32)."""
    l = layout(built, n_nodes=341, total_slots=684, lds_nodes64=1)
    assert l["limit"] == LIMIT == 161280
    assert l["total"] - 1376 + 2816 + 32 == 159808
    assert l["total"] == 158336 and l["fits"] == 1
    for k, v in expected(341, 684, 1).items():
        assert l[k] == v, k


def largest_n(slots_of, n64):
    return max(n for n in range(1, 700) if expected(n, slots_of(n), n64)["total"] <= LIMIT)


@pytest.mark.parametrize("n64", [0, 1])
@pytest.mark.parametrize("emit", [0, 1])
def test_admission_at_the_edges(built, n64, emit):
    def slots_of(n):
        return 2 * n  # about Shirley's ratio

    n_max = max(n for n in range(1, 700) if expected(n, slots_of(n), n64, emit)["total"] <= LIMIT)
    assert 250 < n_max < 500
    for n, fits in ((n_max, 1), (n_max + 1, 0)):
        l = layout(built, n_nodes=n, total_slots=slots_of(n), lds_nodes64=n64, has_emit=emit)
        want = expected(n, slots_of(n), n64, emit)
        for k, v in want.items():
            assert l[k] == v, (n, k)
        assert l["fits"] == fits, (n, l["total"])
    if emit == 0:  # the binary64 bounds cost 48 bytes a node: without them more nodes fit
        assert largest_n(slots_of, 0) > largest_n(slots_of, 1)


def test_admission_small_and_refused(built):
    one = layout(built, n_nodes=1, total_slots=4, lds_nodes64=1)
    assert one["fits"] == 1 and one["leaf"] == 256 and one["sph"] == 272 and one["cat"] == 400 and one["nodes64"] == 416 and one["end"] == 464
    assert one["pool_off"] == 512 and one["total"] == 512 + 6 * PARK
    assert layout(built, n_nodes=0, total_slots=0)["fits"] == 0  # an empty scene
    assert layout(built, n_nodes=1, total_slots=4, mode=1)["fits"] == 0  # Array_leaf keeps the shared image
    # few slots: the record numbers decide (14 bits: 2047 nodes x 8) -- beyond what LDS holds, so the size refuses first
    assert layout(built, n_nodes=MAX_NODES, total_slots=0)["fits"] == 0
    assert layout(built, n_nodes=1, total_slots=4, waves=1)["total"] == 448 + 6 * (64 + 16) * 16  # (no binary64 bounds: the image ends at 416)
