"""Every box decision of the LDS-resident tree walks against the reference's binary64 box test (ptx_walk_next_leaf, include/ptx.h).

ptx_walk_rays and the counting renders observe a walk's OUTCOME: a box wrongly called a miss shows only when the pruned subtree holds
the closest primitive hit, and a ray that grazes a leaf box almost never hits what is inside.  ptx_walk_next_leaf puts a lane of
the production node loops (PtTraverser::walk_asm, walk_asm_oct, the divergent node_step loop; plain and ORIGIN_ZERO) on a node with a
closest hit so far and reports the next leaf whose box test it passes: no leaf is entered, so the answer depends on box decisions
alone -- the binary32 filter's, nested_hit's and slab64's, and through them the magnitude words of both LDS images.

Reference: tests/box_decisions.py's replay of the threaded order on the oracle's own Bbox.is_hit (orc_bbox_is_hit_vec), checked
without a GPU by tests/test_box_decisions.py.  Triples: its families (edges, corners and face points within 4 binary32 ulps; t_max
within binary32 and binary64 ulps of the entry distance, just below it, PT_MAX_FINITE, >= 2^120, 1e-30; origins on faces and inside
boxes; flat and thin boxes, nested and diagonal rays; components of +-0.0, |1/d| to 1e18, subnormal components), from inside the
soup, a few widths outside and 2^22 widths away, each listed for the aimed leaf and every ancestor sharing the targeted faces.

Bar: leaf_out equal to the replay's leaf for EVERY triple.  No tolerance, no triple left out."""
import numpy as np
import pytest

import box_decisions as B
import exact_geometry as X
from test_gpu_edge_cases import make_desc
from test_gpu_walk_rays import admits_oct

pytestmark = pytest.mark.gpu

ERR_ARG, ERR_STATE = -1, -3
PER_FAMILY = 11000  # about 10^5 triples per set with the ancestors
PLACES = {"inside": 0.3, "outside": 4.0, "far": 1000.0}  # |centre| in soup half-widths: where the origin is for the _ZERO walks
# "diagonal": 4 half-widths away along (1, -1, -1).  Seen from the origin every axis of a box then has coordinates and reciprocals of
# one size, so the node's magnitude word is all there is to the margin and the rounding errors of two tying axes are as large
# against it as they get: the placement at which a magnitude word cut to a sixteenth decides wrongly
# (profiles/pr_box_decisions_mutants.txt)
SOUP_PLACES = list(PLACES) + ["diagonal"]


@pytest.fixture(scope="module")
def P():
    import path_tracer_ocaml_amd as P
    assert P.lib().ptx_device_count() >= 1, P.last_error()
    return P


@pytest.fixture(scope="module")
def W():
    from path_tracer_ocaml_amd import abi

    class Walks:
        names = {getattr(abi, k): k[len("PTX_WALK_"):] for k in dir(abi) if k.startswith("PTX_WALK_")}
        SIMD, SIMD_ZERO = [abi.PTX_WALK_SHARED_ASM, abi.PTX_WALK_OCT_ASM], [abi.PTX_WALK_SHARED_ASM_ZERO, abi.PTX_WALK_OCT_ASM_ZERO]
        ARRAY, ARRAY_ZERO = [abi.PTX_WALK_SHARED_DIV], [abi.PTX_WALK_SHARED_DIV_ZERO]
        NONE = [abi.PTX_WALK_PACKET, abi.PTX_WALK_SHARED_ASM_TAIL, abi.PTX_WALK_OCT_ASM_TAIL, abi.PTX_WALK_SHARED_DIV_TAIL]

        @classmethod
        def of(cls, leaf_kind):
            return (cls.SIMD, cls.SIMD_ZERO) if leaf_kind == 0 else (cls.ARRAY, cls.ARRAY_ZERO)
    assert sorted(Walks.SIMD + Walks.SIMD_ZERO + Walks.ARRAY + Walks.ARRAY_ZERO) == sorted(abi.PTX_NEXT_LEAF_WALKS)
    return Walks


def centre_at(scale, place):
    if place == "diagonal":
        return np.array([1.0, -1.0, -1.0]) / np.sqrt(3.0) * scale * 4.0
    return np.array([0.3, -0.2, -0.9]) / np.linalg.norm([0.3, -0.2, -0.9]) * scale * PLACES[place]


def check_decisions(W, g, tree, oracle, walks, t, want=None):
    """leaf_out == the replay's leaf for every triple of `t`, for every walk of `walks`"""
    if want is None:
        want = B.replay(tree, oracle, t.o, t.d, t.node, t.t_max, observable=False).slot
    for w in walks:
        got = g.walk_next_leaf(w, t.o, t.d, t.node, t.t_max)
        wrong = np.nonzero(got != want)[0]
        assert len(wrong) == 0, (W.names[w], len(wrong), [(int(k), int(t.node[k]), int(got[k]), int(want[k]), float(t.t_max[k])) for k in wrong[:5]])
    return want


def check_scene(P, W, oracle, g, leaf_kind, seed, oct=True):
    """both sets of triples (the caller's origins; the origin) through every walk the leaf kind admits"""
    assert g.stats()["traversal_in_lds"]
    if leaf_kind == 0 and oct:
        assert admits_oct(g) and g.stats()["tree_nodes"] <= 2047
    bbox, info, _ = g.tree()
    tree = B.Tree(bbox, info)
    here, zero = W.of(leaf_kind)
    if not oct:
        here, zero = [w for w in here if w != P.abi.PTX_WALK_OCT_ASM], [w for w in zero if w != P.abi.PTX_WALK_OCT_ASM_ZERO]
    with np.errstate(over="ignore", invalid="ignore"):
        t = B.make_triples(tree, seed, PER_FAMILY, zero=False)
        want = check_decisions(W, g, tree, oracle, here, t)
        t0 = B.make_triples(tree, seed + 1, PER_FAMILY, zero=True)
        want0 = check_decisions(W, g, tree, oracle, zero + here, t0)
    assert len(t.node) >= len(B.FAMILIES) * PER_FAMILY and len(t0.node) >= len(B.FAMILIES) * PER_FAMILY
    for s in (want, want0):  # (the walks go somewhere: leaves are reached and the tree is left)
        assert (s >= 0).sum() > 1000 and (s < 0).sum() > 1000
    return tree, t, want


# ---- 1. Simd_leaf: both assembly loops and their origin-zero forms
@pytest.mark.parametrize("place", SOUP_PLACES)
@pytest.mark.parametrize("scale", [B.SCALES[0], B.SCALES[2], B.SCALES[-1]])
@pytest.mark.parametrize("n_spheres", [17, 300])
def test_sphere_soups(P, W, oracle, n_spheres, scale, place):
    rng = np.random.default_rng(3000 + n_spheres)
    d, keep = make_desc(P.abi, spheres=B.sphere_soup(rng, n_spheres, scale, centre_at(scale, place)), leaf_kind=0, cutoff=16)
    g = P.Scene(d, 0, keepalive=keep)
    check_scene(P, W, oracle, g, 0, 100 + n_spheres)
    g.close()


@pytest.mark.parametrize("scale", [3e37, 1e39])
def test_bounds_beyond_binary32_range(P, W, oracle, scale):
    """bounds that overflow in the binary32 image, or whose products do: every visit leaves the assembly loops undecided"""
    rng = np.random.default_rng(77)
    d, keep = make_desc(P.abi, spheres=B.sphere_soup(rng, 120, scale, np.array([0.3, -0.2, -4.0]) * scale, 3.0), leaf_kind=0, cutoff=16)
    g = P.Scene(d, 0, keepalive=keep)
    check_scene(P, W, oracle, g, 0, 5, oct=admits_oct(g))
    g.close()


# ---- 2. Array_leaf: the divergent loop; flat boxes
@pytest.mark.parametrize("place", list(PLACES))
def test_wall_soup(P, W, oracle, place):
    rng = np.random.default_rng(1050)
    d, keep = make_desc(P.abi, tris=B.wall_soup(rng, 200, 1.0, centre_at(1.0, place)), leaf_kind=1, cutoff=4)
    g = P.Scene(d, 0, keepalive=keep)
    tree, _, _ = check_scene(P, W, oracle, g, 1, 9)
    assert ((tree.bbox[:, :3] == tree.bbox[:, 3:]).any(axis=1)).sum() > 20, "the scene was meant to have flat boxes"
    g.close()


def test_cornell(P, W, oracle):
    ptr, keep = X.scene_desc("cornell", oracle, P.abi)
    assert int(ptr.contents.leaf_kind) == 1
    g = P.Scene(ptr, 0, keepalive=keep)
    check_scene(P, W, oracle, g, 1, 13)
    g.close()


# ---- 3. wave shape
@pytest.mark.parametrize("n", [1, 63, 64, 65, 4097])
def test_partial_and_ragged_chunks(P, W, oracle, n):
    """a chunk with one live lane, full chunks, a ragged tail: a triple's answer does not depend on what shares its wave"""
    rng = np.random.default_rng(3300)
    d, keep = make_desc(P.abi, spheres=B.sphere_soup(rng, 300, 1.0, centre_at(1.0, "outside")), leaf_kind=0, cutoff=16)
    g = P.Scene(d, 0, keepalive=keep)
    bbox, info, _ = g.tree()
    tree = B.Tree(bbox, info)
    for zero, walks in ((False, W.SIMD), (True, W.SIMD_ZERO + W.SIMD)):
        t = B.make_triples(tree, 21, 1000, zero)
        pick = np.random.default_rng(n).permutation(len(t.node))[:n]
        t.o, t.d, t.node, t.t_max = (np.ascontiguousarray(a[pick]) for a in (t.o, t.d, t.node, t.t_max))
        check_decisions(W, g, tree, oracle, walks, t)
    g.close()


# ---- 4. refusals
def raw_call(P, g, walk, t, n=None, null=(), o=None, node=None, t_max=None):
    o = np.ascontiguousarray(t.o if o is None else o, dtype=np.float64)
    node = np.ascontiguousarray(t.node if node is None else node, dtype=np.int32)
    t_max = np.ascontiguousarray(t.t_max if t_max is None else t_max, dtype=np.float64)
    n = len(o) if n is None else n
    leaf = np.full(max(n, 1), -7, dtype=np.int32)
    dp, ip = P.abi.c_double_p, P.abi.c_int32_p
    args = [o.ctypes.data_as(dp), t.d.ctypes.data_as(dp), node.ctypes.data_as(ip), t_max.ctypes.data_as(dp), leaf.ctypes.data_as(ip)]
    for k in null:
        args[k] = None
    rc = P.lib().ptx_walk_next_leaf(g._h if g is not None else None, walk, n, *args)
    if rc != 0:  # nothing was launched, nothing written
        assert (leaf == -7).all()
    return rc


def test_walks_a_scene_cannot_take_and_bad_triples(P, W, oracle):
    A = P.abi
    rng = np.random.default_rng(3300)
    d, keep = make_desc(A, spheres=B.sphere_soup(rng, 300, 1.0, centre_at(1.0, "outside")), leaf_kind=0, cutoff=16)
    g = P.Scene(d, 0, keepalive=keep)
    bbox, info, _ = g.tree()
    tree = B.Tree(bbox, info)
    t = B.make_triples(tree, 21, 300, zero=True)
    n_nodes = len(bbox)

    def still_exact():
        check_decisions(W, g, tree, oracle, W.SIMD_ZERO + W.SIMD, t)
    still_exact()
    for w in W.ARRAY + W.ARRAY_ZERO:  # the Array_leaf walk on a Simd_leaf scene
        assert raw_call(P, g, w, t) == ERR_STATE
        assert "Array_leaf" in P.last_error()
    for w in W.NONE + [-1, 10, 1 << 20]:  # the packet walk and the tail cut have no node loop of their own
        assert raw_call(P, g, w, t) == ERR_ARG
        assert "unknown walk" in P.last_error()
    for w in W.SIMD + W.SIMD_ZERO:
        for bad in (-1, n_nodes, n_nodes + 1000, 2 ** 31 - 1, -2 ** 31):  # a node outside the tree, in the last triple
            nodes = t.node.copy()
            nodes[-1] = bad
            assert raw_call(P, g, w, t, node=nodes) == ERR_ARG
            assert "node" in P.last_error()
        for bad in (np.nan, -1e-300, -1.0, -np.inf):
            tm = t.t_max.copy()
            tm[-1] = bad
            assert raw_call(P, g, w, t, t_max=tm) == ERR_ARG
            assert "t_max" in P.last_error()
        for k in range(5):
            assert raw_call(P, g, w, t, null=(k,)) == ERR_ARG
        assert raw_call(P, g, w, t, n=-1) == ERR_ARG
        assert raw_call(P, g, w, t, n=0) == 0
    for w in W.SIMD_ZERO:  # an origin that is not +0.0
        for bad in (-0.0, 1e-300, 5e-324):
            ob = t.o.copy()
            ob[-1, 2] = bad
            assert raw_call(P, g, w, t, o=ob) == ERR_ARG
            assert "+0" in P.last_error()
    assert raw_call(P, None, A.PTX_WALK_SHARED_ASM, t) == ERR_ARG
    with pytest.raises(P.PtxError):
        g.walk_next_leaf(A.PTX_WALK_SHARED_DIV, t.o, t.d, t.node, t.t_max)
    still_exact()
    g.close()
    # a Simd_leaf walk on an Array_leaf scene; a host-only scene
    d, keep = make_desc(A, tris=B.wall_soup(rng, 50, 1.0, centre_at(1.0, "outside")), leaf_kind=1, cutoff=4)
    g = P.Scene(d, 0, keepalive=keep)
    bbox, info, _ = g.tree()
    tree = B.Tree(bbox, info)
    t = B.make_triples(tree, 22, 300, zero=True)
    for w in W.SIMD + W.SIMD_ZERO:
        assert raw_call(P, g, w, t) == ERR_STATE
        assert "Simd_leaf" in P.last_error()
    check_decisions(W, g, tree, oracle, W.ARRAY_ZERO + W.ARRAY, t)
    g.close()
    host = P.Scene(d, -1, keepalive=keep)
    assert raw_call(P, host, A.PTX_WALK_SHARED_DIV, t) == ERR_STATE
    assert "host-only" in P.last_error()
    host.close()


def test_a_scene_walked_from_hbm_takes_none_of_the_walks(P, W, oracle):
    ptr, keep = X.scene_desc("ganesha_150k", oracle, P.abi)
    g = P.Scene(ptr, 0, keepalive=keep)
    try:
        assert not g.stats()["traversal_in_lds"]
        n = 64
        t = B.Triples()
        t.o, t.d, t.node, t.t_max = np.zeros((n, 3)), np.tile([0.0, 0.0, -1.0], (n, 1)), np.zeros(n, dtype=np.int32), np.full(n, B.PT_MAX_FINITE)
        for w in W.SIMD + W.SIMD_ZERO + W.ARRAY + W.ARRAY_ZERO:
            assert raw_call(P, g, w, t) == ERR_STATE, W.names[w]
            assert "HBM" in P.last_error()
    finally:
        g.close()
