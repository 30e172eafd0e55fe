"""The degenerate inputs of tests/bvh_families.py, on the CPU: for every family the product's host builder
(csrc/bvh_build.cpp, through a host-only scene) and the oracle give the same tree bit for bit, both trees are sound
(exact_geometry.check_tree), no tree is deeper than MAX_DEPTH -- and every family still exercises the edge it is there for.
tests/test_gpu_bvh_families.py then ties the GPU builder to the host-only scene of the same descriptors."""
import ctypes as C

import numpy as np
import pytest

import bvh_families as F
import exact_geometry as X


@pytest.fixture(scope="module")
def P():
    import path_tracer_ocaml_amd as P
    return P


_cache = {}


def trees(P, oracle, name, make=None):
    """(desc, host tree, host stats, oracle tree, oracle info) of a family, built once per session"""
    if name not in _cache:
        d, keep = (make or F.FAMILIES[name])()
        h = P.Scene(d, -1, keepalive=keep)
        ht, hs = h.tree(), h.stats()
        h.close()
        o = oracle.Scene(C.pointer(d), keep)
        ot, oi = o.tree(), o.info()
        o.close()
        _cache[name] = (d, keep, ht, hs, ot, oi)
    d, keep, ht, hs, ot, oi = _cache[name]
    return d, ht, hs, ot, oi


@pytest.mark.parametrize("name", list(F.FAMILIES))
def test_host_builder_equals_oracle(P, oracle, name):
    d, ht, hs, ot, oi = trees(P, oracle, name)
    assert F.same_tree(ht, ot) == []
    assert (hs["tree_nodes"], hs["tree_depth"], hs["tree_leaves"], hs["leaf_slots"]) == (oi["nodes"], oi["depth"], oi["leaves"], oi["slots"])
    assert hs["tree_depth"] <= F.MAX_DEPTH
    assert not hs["bvh_built_on_gpu"]
    geo = X.Geometry(C.pointer(d))
    leaf_size = P.lib().ptx_leaf_size()
    assert X.check_tree(geo, *ht, leaf_size) == []
    assert X.check_tree(geo, *ot, leaf_size) == []
    leaves = ht[1][ht[1][:, 0] == 1]
    print(f"{name}: n {geo.n_prims} nodes {hs['tree_nodes']} depth {hs['tree_depth']} leaves {hs['tree_leaves']} "
          f"slots {hs['leaf_slots']} largest leaf {int(leaves[:, 3].max())}")


# ---------------------------------------------------------------- what each family is for
def test_coincident_family_is_one_leaf(P, oracle):
    _, ht, hs, _, _ = trees(P, oracle, "coincident-9000")
    assert hs["tree_nodes"] == 1 and hs["tree_leaves"] == 1
    assert ht[1][0, 0] == 1 and ht[1][0, 2] == 0 and ht[1][0, 3] == F.COINCIDENT_N
    assert np.array_equal(ht[2], np.arange(F.COINCIDENT_N))


def test_duplicates_keep_their_copies_together(P, oracle):
    for name in ("duplicates-700x13", "duplicates-700x13-simd16"):
        _, ht, _, _, _ = trees(P, oracle, name)
        info, order = ht[1], ht[2]
        for leaf in info[info[:, 0] == 1]:
            slots = order[leaf[2]:leaf[2] + leaf[3]]
            prims = slots[slots >= 0]
            assert (np.unique(prims // 13, return_counts=True)[1] == 13).all()


def test_zero_range_axes_are_never_split(P, oracle):
    for name, dead in (("line-x-9000", (1, 2)), ("plane-xy-9000", (2,)), ("flat-triangles-5000", (2,)),("point-triangles-5000", (2,)),
                       ("concentric-9000", (0, 1, 2))):
        d, ht, _, _, _ = trees(P, oracle, name)
        pb = X.Geometry(C.pointer(d)).prim_boxes()
        cen = 0.5 * (pb[:, :3] + pb[:, 3:])
        for a in dead:
            assert cen[:, a].min() == cen[:, a].max(), (name, a)
        inner = ht[1][ht[1][:, 0] == 0]
        assert not np.isin(inner[:, 1], dead).any(), name
        assert (len(inner) == 0) == (len(dead) == 3), name


def _area(b):
    """Bbox.surface_area, bbox.ml:33-38 (the fused form agrees wherever the products are exact, see lattice_points)"""
    x, y, z = b[3] - b[0], b[4] - b[1], b[5] - b[2]
    return 2.0 * (x * y + (y * z + z * x))


def _axis_candidates(boxes, axis, num_bins):
    """Proposal.propose_split_one_axis (shape_tree.ml:91-139) restated: [(p, n_left, cost)] for every split index p with
    elements on both sides, in float64"""
    cen = 0.5 * (boxes[:, axis] + boxes[:, axis + 3])
    scale = float(num_bins) * (1.0 - 1e-6) / (cen.max() - cen.min())
    if not np.isfinite(scale):
        return []
    b = (scale * (cen - cen.min())).astype(np.int64)  # Float.to_int truncates; all arguments are >= 0
    union = lambda s: np.concatenate([boxes[s, :3].min(0), boxes[s, 3:].max(0)])
    total = _area(union(np.ones(len(boxes), bool)))
    out = []
    for p in range(num_bins - 1):
        left = b <= p
        nl, nr = int(left.sum()), int((~left).sum())
        if nl == 0 or nr == 0:
            continue
        out.append((p, nl, 0.25 + (nl * _area(union(left)) + nr * _area(union(~left))) * 1.0 / total))
    return out


def _subtree_prims(info, order, k):
    stack, prims = [k], []
    while stack:
        leaf, _, a, b = (int(v) for v in info[stack.pop()])
        if leaf:
            prims += [p for p in order[a:a + b].tolist() if p >= 0]
        else:
            stack += [a, b]
    return np.array(sorted(prims))


@pytest.mark.parametrize("name", list(F.LATTICES))
def test_lattice_splits_are_decided_by_the_tie_rules(P, oracle, name):
    """Costs recomputed from the restated formula for the first nodes of the tree: the chosen axis is the FIRST of the axes
    that share the lowest cost (X before Y before Z), the chosen index is the HIGHEST p among equal costs, and the lattice
    does tie: at least one of these nodes has a rival axis at exactly the same cost, and on the 21-cube (an odd count:
    10 | 11 and 11 | 10 layers cost the same) a rival split of the same axis that divides the elements differently."""
    d, ht, _, _, _ = trees(P, oracle, name)
    _, info, order = ht
    pb = X.Geometry(C.pointer(d)).prim_boxes()
    axis_rivals = index_rivals = 0
    todo, seen = [0], 0
    while todo and seen < 7:
        k = todo.pop(0)
        leaf, axis, lhs, rhs = (int(v) for v in info[k])
        if leaf:
            continue
        seen += 1
        todo += [lhs, rhs]
        prims = _subtree_prims(info, order, k)
        per_axis = [_axis_candidates(pb[prims], a, d.num_bins) for a in range(3)]
        low = [min(c[2] for c in cand) if cand else np.inf for cand in per_axis]
        best = min(low)
        assert axis == low.index(best), f"node {k}: axis {axis}, costs {low}"
        axis_rivals += sum(1 for a in range(3) if a != axis and low[a] == best)
        ties = [c for c in per_axis[axis] if c[2] == best]
        n_left = len(_subtree_prims(info, order, lhs))
        assert n_left == ties[-1][1], f"node {k}: {n_left} elements on the left, equal-cost candidates {ties}"
        index_rivals += len({c[1] for c in ties}) > 1
    assert axis_rivals >= 1
    if name == "lattice-21x21x21":
        assert index_rivals >= 1


def test_collinear_family_has_no_area_and_every_cost_is_nan(P, oracle):
    d, ht, hs, _, _ = trees(P, oracle, "collinear-triangles-150")
    pb = X.Geometry(C.pointer(d)).prim_boxes()
    root = np.concatenate([pb[:, :3].min(0), pb[:, 3:].max(0)])
    assert _area(root) == 0.0 and root[3] > root[0]
    with np.errstate(invalid="ignore"):
        cand = _axis_candidates(pb, 0, d.num_bins)
    assert len(cand) > 1 and all(np.isnan(c[2]) for c in cand)
    assert hs["tree_nodes"] > 1 and (ht[1][ht[1][:, 0] == 0][:, 1] == 0).all()


def test_signed_zero_families_hold_the_zeros_they_promise(P, oracle):
    want = {"signed-zero-mixed": (slice(0, 3), True), "signed-zero-negative": (slice(0, 3), False), "signed-zero-mirror": (slice(3, 6), True)}
    for name, (cols, mixed) in want.items():
        d, ht, _, _, _ = trees(P, oracle, name)
        pb = X.Geometry(C.pointer(d)).prim_boxes()
        z = pb[:, cols][pb[:, cols] == 0.0]
        assert len(z) == 4200 and not (np.delete(pb, np.r_[cols], axis=1) == 0.0).any()
        assert np.signbit(z).any() and (not np.signbit(z).all()) == mixed
        n_zero, n_neg = F.zero_bounds(ht[0])
        assert n_zero > 1000 and n_neg > 0 and (n_neg < n_zero) == mixed
        print(f"{name}: {n_zero} zero bounds in the host tree, {n_neg} of them -0.0")


def test_alternation_order_decides_the_sign_of_a_union(P, oracle):
    """Float.min and Float.max keep the second argument on a tie: two scenes that differ only in which zero comes first
    get trees that differ only in the sign bits of zero-valued bounds -- and the host builder follows the oracle in both."""
    got = []
    for order in ((0, 1), (1, 0)):
        _, ht, _, ot, _ = trees(P, oracle, f"alternating-{order}", lambda: F.alternating_zero_triangles(order))
        assert F.same_tree(ht, ot) == []
        got.append(ht)
    (b0, i0, o0), (b1, i1, o1) = got
    assert np.array_equal(i0, i1) and np.array_equal(o0, o1) and np.array_equal(b0, b1)  # equal as numbers
    s0, s1 = np.signbit(b0[b0 == 0.0]), np.signbit(b1[b1 == 0.0])
    print(f"zero bounds {len(s0)}, negative {int(s0.sum())} and {int(s1.sum())}")
    assert s0.any() and not s0.all() and s1.any() and not s1.all()
    assert not np.array_equal(s0, s1)
    # no reduction that ignores the order could give both: the union of all 40 boxes is the same set either way
    assert np.signbit(b0[0, 1]) != np.signbit(b1[0, 1])


def test_sizes_sit_on_the_class_boundaries():
    """the constants of csrc/bvh_build_gpu.inc the size edges are chosen around"""
    import os
    import re
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "path_tracer_ocaml_amd", "csrc", "bvh_build_gpu.inc")).read()
    c = {k: int(v) for k, v in re.findall(r"#define (BVH_SMALL_MAX|BVH_BIG_MIN|BVH_TILE|BVH_MAX_BINS)\s+(\d+)", src)}
    assert re.search(r"private_bins = n >= 2048;", src)
    for edge in (c["BVH_SMALL_MAX"], 2048 - 1, c["BVH_BIG_MIN"] - 1, c["BVH_BIG_MIN"], 5 * c["BVH_TILE"]):
        assert edge in F.SIZE_EDGES and edge + 1 in F.SIZE_EDGES
    assert c["BVH_MAX_BINS"] in F.BIN_COUNTS and c["BVH_MAX_BINS"] + 1 in F.BIN_COUNTS
    assert 4096 in F.SIZE_EDGES and 4095 in F.SIZE_EDGES  # the automatic choice of builder (ptx.h, `reserved`)
