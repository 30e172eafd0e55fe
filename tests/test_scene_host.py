"""Scene construction (path_tracer_ocaml_amd/csrc/scene_host.cpp) without a GPU, under AddressSanitizer + UndefinedBehaviorSanitizer:
host_asan_driver's `arrays` mode assembles a scene with the code the library ships and prints digests of everything it made.

* tests/golden/scene_arrays.json pins every array and scalar to what scene_build produced BEFORE it was split into that unit.
  It was recorded from the parent commit's library (hipcc's host compiler, -O3), patched for the occasion so that a host-only
  scene ran past its early return and printed the same digests; the test runs g++ -O1 under the sanitizers.  Contraction is off
  in both, so the two compilers must agree to the bit.
* The threading of the node images (skip32 + nodes32, nodes32o, top_nodes + skip32_top, the 16-bit skip) is checked against the
  tree itself: a recursive near-child-first descent (shape_tree.ml:209) gives the order every walk must follow."""
import json
import os

import numpy as np
import pytest

from test_sanitizers import ENV, ROOT, built, run_clean  # noqa: F401  (built: the `make asan` fixture)

FIXTURE = json.load(open(os.path.join(ROOT, "tests", "golden", "scene_arrays.json")))
END = -1
PT_TOP_FLAG, PT_OCT_END, PT_OCT_LEAF_TAG, PT_OCT_LEAF_FIRST_BITS = 0x20000000, 0x80000000, 0x40000000, 22
NODE = np.dtype([("mn", "<f8", 3), ("mx", "<f8", 3), ("a", "<u4"), ("b", "<u4"), ("pad", "<u4", 2)])


def arrays(built, scene, options=None, dump=None):
    cmd = [os.path.join(built, "host_asan_driver"), "arrays", scene] + [f"{k}={v}" for k, v in (options or {}).items()]
    return json.loads(run_clean(cmd + ([f"dump={dump}"] if dump else []), timeout=900))


def case_id(case):
    return case["scene"] + "".join(f"-{k}{v}" for k, v in case["options"].items())


def fixture_of(scene, **options):
    return next(c["arrays"] for c in FIXTURE if c["scene"] == scene and c["options"] == options)


@pytest.mark.parametrize("case", FIXTURE, ids=case_id)
def test_arrays_equal_the_parent_commits(built, case):
    got = arrays(built, case["scene"], case["options"])
    want = case["arrays"]
    for group in ("vectors", "dev"):
        for name in want[group]:
            assert got[group][name] == want[group][name], (group, name)
    assert got == want


def test_the_fixture_is_not_trivial():
    assert [case_id(c) for c in FIXTURE] == [
        "shirley", "shirley_array", "cornell", "cornell_lamp", "ganesha", "ganesha_150k", "ganesha-oct_image0", "ganesha-top_nodes1",
        "ganesha-top_nodes64", "ganesha-top_nodes1023", "cornell-tri_frame0", "ganesha-bin_key0", "ganesha-bin_key1", "ganesha-bin_key2"]
    for scene in ("ganesha", "ganesha_150k"):  # 3000 triangles (1739 nodes: beyond the LDS image's 712) and the benchmark's mesh
        v = fixture_of(scene)["vectors"]
        assert v["nodes32o"][0] == 64 * v["nodes"][0] > 0 and v["top_nodes"][0] > 0 and v["skip32_top"][0] == v["skip32"][0] > 0
    assert fixture_of("ganesha_150k")["n_prims"] > 140000
    c = fixture_of("cornell")
    assert c["vectors"]["tri_frame"][0] > 0 and c["light_table"][0] == 14 * c["n_emissive_tris"] > 0
    assert fixture_of("cornell", tri_frame=0)["vectors"]["tri_frame"][0] == 0
    assert fixture_of("ganesha", oct_image=0)["vectors"]["nodes32o"][0] == 0
    assert len({fixture_of("ganesha", top_nodes=k)["vectors"]["top_nodes"][1] for k in (1, 64, 1023)}) == 3
    keys = [(d["sort_by_elevation"], d["sort_by_root"]) for d in (fixture_of("ganesha", bin_key=k)["dev"] for k in (0, 1, 2))]
    assert keys == [(0, 0), (1, 0), (0, 1)]
    m = fixture_of("cornell_lamp")["vectors"]  # spheres and triangles in one tree
    assert m["sph"][0] > 0 and m["tri"][0] > 0


# ---- threading against the tree ----
def descent(nodes, o):
    """The nodes in the order of a recursive descent that takes the near child first (lhs where bit `axis` of the octant is set), and
    for every node the node that order visits right after its subtree (END: none)."""
    order, after, todo = [], np.full(len(nodes), END, dtype=np.int64), [(0, END)]
    while todo:
        k, nxt = todo.pop()
        order.append(k)
        after[k] = nxt
        axis = int(nodes["b"][k]) >> 30
        if axis == 3:
            continue
        lhs, rhs = int(nodes["a"][k]), int(nodes["b"][k]) & 0x3FFFFFFF
        near, far = (lhs, rhs) if (o >> axis) & 1 else (rhs, lhs)
        todo.append((far, nxt))
        todo.append((near, far))
    return order, after


def check_walk(nodes, o, start, visit, node_of):
    """visit(ref) = (node, the reference a hit leads to, the one a miss leads to); node_of(ref) = the node a reference names (END:
    the walk is over).  (a) every box test a hit: the nodes of descent(), in its order, then the end; (b) every miss link: what
    follows the node's subtree."""
    order, after = descent(nodes, o)
    ref, seen = start, []
    while node_of(ref) != END:
        assert len(seen) < len(order), "the walk does not end"
        k, hit, miss = visit(ref)
        assert k == node_of(ref)
        assert node_of(miss) == after[k], (o, k)
        seen.append(k)
        ref = hit
    assert seen == order, o


def load(dump, name, dtype):
    return np.fromfile(os.path.join(dump, name + ".bin"), dtype=dtype)


@pytest.mark.parametrize("scene", ["ganesha", "shirley_array"])
def test_threading_follows_the_tree(built, tmp_path, scene):
    arrays(built, scene, dump=str(tmp_path))
    nodes = load(tmp_path, "nodes", NODE)
    n = len(nodes)
    skip32, skip16 = load(tmp_path, "skip32", "<u4").reshape(n, 8), load(tmp_path, "skip", "<u2")
    nodes32, nodes32o = load(tmp_path, "nodes32", "<u4").reshape(n, 8), load(tmp_path, "nodes32o", "<u4").reshape(-1, 8)
    top, skip32_top = load(tmp_path, "top_nodes", "<u4").reshape(-1, 16), load(tmp_path, "skip32_top", "<u4").reshape(-1, 8)
    top_skip = load(tmp_path, "top_nodes", "<u2").reshape(-1, 32)[:, 16:24]  # words 8 .. 11 of a top record
    assert len(skip16) == 8 * n  # both trees have fewer than 65535 nodes
    skip16 = skip16.reshape(n, 8)
    if scene == "ganesha":
        assert len(nodes32o) == 8 * n and len(top) > 2 and len(skip32_top) == n
    assert np.array_equal(nodes32[:, 6], nodes["a"])
    leaf = (nodes["b"] >> 30) == 3
    assert np.array_equal(nodes32[~leaf, 7], nodes["b"][~leaf])
    assert np.array_equal(nodes32[leaf, 7], (nodes["b"][leaf] & 0x7FFF) | ((nodes["pad"][leaf, 0] & 0x7FFF) << 15) | (3 << 30))

    def near32(k, o):  # the near child of an inner node by the words of nodes32
        a, b = int(nodes32[k, 6]), int(nodes32[k, 7])
        return a if (o >> (b >> 30)) & 1 else b & 0x3FFFFFFF

    for o in range(8):
        for table, none in ((skip32, 0xFFFFFFFF), (skip16, 0xFFFF)):
            def plain(ref, none=none):
                return END if ref == none else ref

            def visit(k, table=table):
                return k, (int(table[k, o]) if leaf[k] else near32(k, o)), int(table[k, o])
            check_walk(nodes, o, 0, visit, plain)

        if len(nodes32o):
            base = o * n

            def oct_node(ref):
                assert ref == PT_OCT_END or base <= ref < base + n  # links carry the octant's base
                return END if ref == PT_OCT_END else ref - base

            def oct_visit(ref):
                w, k = nodes32o[ref], ref - base
                if leaf[k]:  # the leaf's packet in word 6; afterwards the walk continues at word 7
                    assert int(w[6]) >> 30 == PT_OCT_LEAF_TAG >> 30
                    assert int(w[6]) & ((1 << PT_OCT_LEAF_FIRST_BITS) - 1) == nodes["a"][k]
                    assert (int(w[6]) >> PT_OCT_LEAF_FIRST_BITS) & 255 == nodes["pad"][k, 0]
                    return k, int(w[7]), int(w[7])
                return k, int(w[6]), int(w[7])
            check_walk(nodes, o, base, oct_visit, oct_node)

        if len(top):
            def top_node(ref):
                if ref == 0xFFFFFFFF:
                    return END
                if ref & PT_TOP_FLAG:
                    assert (ref ^ PT_TOP_FLAG) % 64 == 0
                    return int(top[(ref ^ PT_TOP_FLAG) // 64, 12])  # w[12] names the node
                return ref

            def top_visit(ref):
                if not ref & PT_TOP_FLAG:  # below the top image: nodes32 and skip32_top
                    return ref, (int(skip32_top[ref, o]) if leaf[ref] else near32(ref, o)), int(skip32_top[ref, o])
                w = top[(ref ^ PT_TOP_FLAG) // 64]
                k, sk = int(w[12]), int(top_skip[(ref ^ PT_TOP_FLAG) // 64, o])
                miss = 0xFFFFFFFF if sk == 0xFFFF else PT_TOP_FLAG | sk  # 16-bit byte offsets into the top image
                if leaf[k]:
                    assert int(w[6]) == nodes["a"][k] and int(w[7]) == nodes32[k, 7]
                    return k, miss, miss
                lhs, rhs, axis = int(w[6]), int(w[7]) & 0x3FFFFFFF, int(w[7]) >> 30
                assert top_node(lhs) == nodes["a"][k] and top_node(rhs) == nodes["b"][k] & 0x3FFFFFFF and axis == nodes["b"][k] >> 30
                return k, (lhs if (o >> axis) & 1 else rhs), miss
            assert int(top[0, 12]) == 0
            check_walk(nodes, o, PT_TOP_FLAG | 0, top_visit, top_node)
    if len(top):  # a node with a top slot is never referred to by its plain index
        assert not np.isin(skip32_top, top[:, 12]).any()
