"""Support for tests/test_box_decisions.py and tests/test_gpu_box_decisions.py: the reference of ptx_walk_next_leaf and the
(ray, node, t_max) triples it is asked about.

REPLAY.  Given the tree of ptx_scene_tree, a ray, a start node and t_max: follow the threaded order the LDS images encode (near child
first on a hit, skip link on a miss -- tests/test_scene_host.py's `descent` gives both links per octant), decide EVERY box with the
oracle's own Bbox.is_hit in binary64 (orc_bbox_is_hit_vec: a loop over orc_bbox_is_hit; nothing here restates the box test), return
the first slot of the first leaf whose box is hit, or -1.  All triples are replayed in lockstep, one visit per turn.
Beside the leaf: whether the FIRST decision is observable (flipping it changes the returned leaf), what that decision was, and how
many boxes were tested.

TRIPLES.  Deterministic, seeded families (FAMILIES); each aims at ONE leaf box's decision and lists that leaf plus every ancestor
whose box shares the targeted face coordinates (the same ray is as close a call for them).  With zero=True every origin is +0.0 and
the families are aimed from there (the _ZERO walks): the soup's placement then decides whether the origin is inside, near or far."""
import numpy as np

from test_gpu_fuzz import SCALES, leaf_boxes, ray_mix, sphere_soup, wall_soup  # noqa: F401  (re-exported: the scenes of both modules)
from test_gpu_walk_rays import dirs_from_origin
from test_scene_host import descent

END = -1
PT_MAX_FINITE = 1.7976931348623157e308
U32 = 2.0 ** -24  # "a binary32 ulp of its magnitude", as ray_mix counts them
FAMILIES = ("mix", "edges", "t_max", "origin", "thin", "directions")


class Tree:
    """ptx_scene_tree's arrays, the links of the threaded walk per octant, and every node's parent"""

    def __init__(self, bbox, info):
        n = len(bbox)
        self.bbox = np.ascontiguousarray(bbox, dtype=np.float64)
        self.leaf = info[:, 0] == 1
        self.first_slot = np.where(self.leaf, info[:, 2], -1).astype(np.int64)
        axis = np.where(self.leaf, 3, info[:, 1]).astype(np.int64)
        nodes = np.zeros(n, dtype=[("a", "<u4"), ("b", "<u4")])  # PtNode's link words, as `descent` reads them
        nodes["a"] = info[:, 2]
        nodes["b"] = (axis << 30) | info[:, 3].astype(np.int64)
        self.hit = np.full((8, n), END, dtype=np.int64)   # where a hit on an inner node leads (a leaf: the walk holds it)
        self.miss = np.full((8, n), END, dtype=np.int64)  # where a miss leads, and the end of a leaf
        self.parent = np.full(n, END, dtype=np.int64)
        inner = np.nonzero(~self.leaf)[0]
        lhs, rhs = info[inner, 2].astype(np.int64), info[inner, 3].astype(np.int64)
        self.parent[lhs] = inner
        self.parent[rhs] = inner
        for o in range(8):
            order, after = descent(nodes, o)
            assert sorted(order) == list(range(n))
            self.miss[o] = after
            self.hit[o, inner] = np.where((o >> axis[inner]) & 1, lhs, rhs)
        self.leaves = np.nonzero(self.leaf)[0]
        root = self.bbox[0]
        self.centre = (root[:3] + root[3:]) / 2
        self.scale = float((root[3:] - root[:3]).max() / 2)


def octant(d):
    """PtTraverser::begin's `dirs` (shape_tree.ml:201): bit a set where component a >= 0 (-0.0 included, a NaN not)"""
    d = np.asarray(d)
    return (d[:, 0] >= 0.0) * 1 + (d[:, 1] >= 0.0) * 2 + (d[:, 2] >= 0.0) * 4


def walk(tree, O, o, d, start, t_max):
    """from `start` (END: nothing to do) to the first leaf whose box is hit -> (that leaf's NODE or END, boxes tested, first decision)"""
    n = len(start)
    oc = octant(d)
    cur = np.asarray(start, dtype=np.int64).copy()
    out = np.full(n, END, dtype=np.int64)
    tests = np.zeros(n, dtype=np.int64)
    first = np.zeros(n, dtype=bool)
    act = np.nonzero(cur >= 0)[0]
    turn = 0
    while len(act):
        assert turn <= len(tree.bbox), "the threaded order only goes forward"
        k = cur[act]
        h = O.bbox_is_hit_vec(tree.bbox[k], o[act], d[act], np.zeros(len(act)), t_max[act])
        tests[act] += 1
        if turn == 0:
            first[act] = h
        got = h & tree.leaf[k]
        out[act[got]] = k[got]
        nxt = np.where(h, tree.hit[oc[act], k], tree.miss[oc[act], k])
        cur[act] = nxt
        act = act[~got & (nxt >= 0)]
        turn += 1
    return out, tests, first


class Replay:
    pass


def replay(tree, O, o, d, node, t_max, observable=True):
    """.slot: what ptx_walk_next_leaf must return; .leaf_node; .tests; .first (the first decision, binary64); .observable"""
    o, d = np.ascontiguousarray(o, dtype=np.float64), np.ascontiguousarray(d, dtype=np.float64)
    node, t_max = np.asarray(node, dtype=np.int64), np.ascontiguousarray(t_max, dtype=np.float64)
    r = Replay()
    r.leaf_node, r.tests, r.first = walk(tree, O, o, d, node, t_max)
    r.slot = np.where(r.leaf_node >= 0, tree.first_slot[r.leaf_node], -1).astype(np.int32)
    if observable:
        oc = octant(d)
        on_hit = np.where(tree.leaf[node], node, walk(tree, O, o, d, np.where(tree.leaf[node], END, tree.hit[oc, node]), t_max)[0])
        on_miss = walk(tree, O, o, d, tree.miss[oc, node], t_max)[0]
        assert np.array_equal(r.leaf_node, np.where(r.first, on_hit, on_miss))
        r.observable = on_hit != on_miss
    return r


def chain_tests(tree, O, o, d):
    """boxes tested by a whole walk from the root that enters no leaf's primitives' hit (t_max stays PT_MAX_FINITE): the replay
    chained leaf by leaf to the end of the tree"""
    n = len(o)
    t_max = np.full(n, PT_MAX_FINITE)
    oc = octant(d)
    start = np.zeros(n, dtype=np.int64)
    total = 0
    while (start >= 0).any():
        leaf, tests, _ = walk(tree, O, np.ascontiguousarray(o), np.ascontiguousarray(d), start, t_max)
        total += int(tests.sum())
        start = np.where(leaf >= 0, tree.miss[oc, np.maximum(leaf, 0)], END)
    return total


# ---------------------------------------------------------------------------------------------------------------- the triples
class Family:
    def __init__(self, o, d, node, t_max, faces=None):
        self.o, self.d, self.node, self.t_max = o, d, np.asarray(node, dtype=np.int64), t_max
        self.faces = faces  # (n, 6) bool over (min xyz, max xyz): the targeted face coordinates; None: no ancestors listed


def views(rng, n, tree, zero):
    """origins inside the soup, a few widths outside, and 2^22 widths away (far away a box is narrower than a binary32 ulp of its
    distance) -> (origins, the kind 0 / 1 / 2 of each)"""
    kind = rng.integers(0, 3, n)
    if zero:
        return np.zeros((n, 3)), kind
    o = tree.centre + rng.uniform(-1.0, 1.0, (n, 3)) * tree.scale * np.where(kind[:, None] == 1, 40.0, 1.5)
    far = kind == 2
    o[far] = tree.centre + rng.normal(size=(far.sum(), 3)) * tree.scale * 2.0 ** 22
    return o, kind


def pick(rng, tree, n):
    leaf = tree.leaves[rng.integers(0, len(tree.leaves), n)]
    bx = tree.bbox[leaf]
    return leaf, bx[:, :3], bx[:, 3:]


def rescale(rng, d):
    with np.errstate(over="ignore"):
        return d * 10.0 ** rng.uniform(-3.0, 3.0, (len(d), 1))  # (no walk asks for unit directions)


def between_binary32(rng, d, share=2):
    """every `share`-th direction with each component moved to 0.49 binary32 ulps above or below a binary32 number: the filter's
    (float)d then carries nearly its whole rounding error, with a sign per axis (opposite signs on two tying axes add up)"""
    with np.errstate(over="ignore", invalid="ignore"):
        v = d.astype(np.float32)
        moved = v.astype(np.float64) + rng.choice([-0.49, 0.49], d.shape) * np.spacing(np.abs(v)).astype(np.float64)
    ok = np.isfinite(moved) & (v != 0.0) & (np.arange(len(d)) % share == 0)[:, None]
    return np.where(ok, moved, d)


def feature_points(rng, lo, hi, kinds):
    """a point of each box on a face (kinds 2), an edge (0) or a corner (1), moved by -4 .. +4 binary32 ulps of its magnitude
    -> (points, the (n, 6) mask of the face coordinates it lies on)"""
    n = len(lo)
    rows = np.arange(n)
    a1 = rng.integers(0, 3, n)
    a2 = (a1 + 1 + rng.integers(0, 2, n)) % 3
    a3 = 3 - a1 - a2
    on = np.zeros((n, 3), dtype=bool)
    on[rows, a1] = True
    on[rows, a2] = kinds <= 1
    on[rows, a3] = kinds == 1
    side = rng.integers(0, 2, (n, 3)).astype(bool)
    pt = np.where(on, np.where(side, hi, lo), lo + (hi - lo) * rng.uniform(0.0, 1.0, (n, 3)))
    pt = pt + np.abs(pt) * rng.integers(-4, 5, (n, 3)) * U32
    return pt, np.concatenate([on & ~side, on & side], axis=1)


def slab_entry(lo, hi, o, d):
    """the reference's entry and exit distances (bbox.ml:40-56) in numpy -- to AIM t_max with, never to judge anything"""
    with np.errstate(all="ignore"):
        inv = 1.0 / d
        t0, t1 = (lo - o) * inv, (hi - o) * inv
        near, far = np.minimum(t0, t1), np.maximum(t0, t1)
        return near.max(axis=1), np.argmax(near, axis=1), far.min(axis=1)


def fam_mix(rng, tree, n, zero):
    """ray_mix's rays (dirs_from_origin's from the origin) against the root and against nodes chosen at random"""
    if zero:
        _, mixed = ray_mix(rng, n, tree.scale, tree.centre, tree.bbox)
        d = dirs_from_origin(rng, n, tree.scale, tree.centre, tree.bbox, mixed)
        o = np.zeros((n, 3))
    else:
        o, d = ray_mix(rng, n, tree.scale, tree.centre, tree.bbox)
    node = np.where(rng.integers(0, 2, n) == 0, 0, rng.integers(0, len(tree.bbox), n))
    return Family(o, d, node, np.full(n, PT_MAX_FINITE))


def fam_edges(rng, tree, n, zero):
    leaf, lo, hi = pick(rng, tree, n)
    pt, faces = feature_points(rng, lo, hi, rng.integers(0, 3, n))
    o, _ = views(rng, n, tree, zero)
    return Family(o, between_binary32(rng, rescale(rng, pt - o)), leaf, np.full(n, PT_MAX_FINITE), faces)


def t_max_variants(rng, base):
    """t_max around `base` (> 0): +-0..8 binary32 ulps, +-1..4 binary64 ulps, just below, PT_MAX_FINITE, >= 2^120, 1e-30, exact"""
    n = len(base)
    v = rng.integers(0, 7, n)
    t = base.copy()
    t = np.where(v == 0, base * (1.0 + rng.integers(-8, 9, n) * U32), t)
    steps, up = rng.integers(1, 5, n), rng.integers(0, 2, n) == 1
    moved = base.copy()
    for s in range(1, 5):
        moved = np.where(steps >= s, np.nextafter(moved, np.where(up, np.inf, 0.0)), moved)
    t = np.where(v == 1, moved, t)
    t = np.where(v == 2, base * (1.0 - 10.0 ** rng.uniform(-6.0, -3.0, n)), t)
    t = np.where(v == 3, PT_MAX_FINITE, t)
    t = np.where(v == 4, rng.choice([2.0 ** 120, 2.0 ** 121, 2.0 ** 200, 1e300], n), t)
    t = np.where(v == 5, 1e-30, t)
    return np.where(np.isfinite(t) & (t >= 0.0), t, PT_MAX_FINITE)


def fam_t_max(rng, tree, n, zero):
    """rays aimed inside a leaf box, t_max around the box's binary64 entry distance (the exit distance where the origin is inside)"""
    leaf, lo, hi = pick(rng, tree, n)
    pt = lo + (hi - lo) * rng.uniform(0.05, 0.95, (n, 3))
    o, _ = views(rng, n, tree, zero)
    d = rescale(rng, pt - o)
    te, am, tx = slab_entry(lo, hi, o, d)
    base = np.where(te > 0.0, te, tx)
    base = np.where(np.isfinite(base) & (base > 0.0), base, 1.0)
    faces = np.zeros((n, 6), dtype=bool)
    faces[np.arange(n), am + 3 * (d[np.arange(n), am] < 0.0)] = True  # the entry face
    return Family(o, d, leaf, t_max_variants(rng, base), faces)


def fam_origin(rng, tree, n, zero):
    """origins exactly on a face of a leaf box, +-4 ulps around it (max(near, 0) clamps), and inside the box.  From the origin: rays
    through such points with a power of two for a length, so that the point lies at t = 2^-j exactly, and t_max around that"""
    leaf, lo, hi = pick(rng, tree, n)
    rows = np.arange(n)
    ax, side = rng.integers(0, 3, n), rng.integers(0, 2, n)
    mode = rng.choice([0, 1, 1, 2], n)  # on the face, around it, inside
    p = lo + (hi - lo) * rng.uniform(0.0, 1.0, (n, 3))
    coord = np.where(side == 1, hi[rows, ax], lo[rows, ax])
    k = rng.integers(1, 5, n) * rng.choice([-1, 1], n)
    p[rows, ax] = np.where(mode == 0, coord, np.where(mode == 1, coord + np.abs(coord) * k * U32, p[rows, ax]))
    faces = np.zeros((n, 6), dtype=bool)
    faces[rows, ax + 3 * side] = True
    if zero:
        j = rng.integers(-3, 4, n).astype(np.float64)
        return Family(np.zeros((n, 3)), p * 2.0 ** j[:, None], leaf, t_max_variants(rng, 2.0 ** -j), faces)
    d = rescale(rng, rng.normal(size=(n, 3)) * tree.scale)
    ext = np.maximum((hi - lo).max(axis=1), tree.scale * 1e-9) / np.abs(d).max(axis=1)
    t_max = np.where(rng.integers(0, 3, n) == 0, ext * rng.uniform(0.0, 2.0, n), PT_MAX_FINITE)
    t_max = np.where(rng.integers(0, 8, n) == 0, 1e-30, t_max)
    return Family(p, d, leaf, np.where(np.isfinite(t_max), t_max, PT_MAX_FINITE), faces)


def fam_thin(rng, tree, n, zero):
    """a leaf box's thinnest axis k (a wall's: flat).  Rays that cross the k-slab well inside the other two (nested_hit's case), the
    same aimed beside the box or stopped short of it, and rays through an edge of a k-face along its diagonal (|d_k| = |d_j|: two
    axes near-tie, binary64 must decide)"""
    leaf, lo, hi = pick(rng, tree, n)
    rows = np.arange(n)
    ext = hi - lo
    k = np.argmin(ext, axis=1)
    j = (k + 1 + rng.integers(0, 2, n)) % 3
    i = 3 - k - j
    sub = rng.integers(0, 4, n)  # 0 nested, 1 nested and stopped short, 2 beside the box, 3 diagonal
    pt = lo + ext * rng.uniform(0.3, 0.7, (n, 3))
    beside = sub == 2
    pt[rows[beside], j[beside]] = (hi[rows, j] + np.maximum(ext[rows, j], tree.scale * 1e-6) * rng.uniform(0.05, 1.0, n))[beside]
    diag = sub == 3
    sk, sj = rng.integers(0, 2, n), rng.integers(0, 2, n)
    pt[rows[diag], k[diag]] = np.where(sk == 1, hi[rows, k], lo[rows, k])[diag]
    pt[rows[diag], j[diag]] = np.where(sj == 1, hi[rows, j], lo[rows, j])[diag]
    pt = np.where(diag[:, None], pt + np.abs(pt) * rng.integers(-4, 5, (n, 3)) * U32, pt)
    # direction: the k component leads; across the box the ray moves sideways by at most a fifth of the box (nested), or as far
    # along j as along k (the diagonal)
    size = np.maximum(ext.max(axis=1), tree.scale * 1e-6)
    d = np.zeros((n, 3))
    d[rows, k] = size * rng.choice([-1.0, 1.0], n)
    ratio = np.minimum(1.0, 0.2 * ext / np.maximum(ext[rows, k], size * 1e-12)[:, None])
    d[rows, j] = size * rng.uniform(-1.0, 1.0, n) * ratio[rows, j]
    d[rows, i] = size * rng.uniform(-1.0, 1.0, n) * ratio[rows, i]
    d[rows[diag], j[diag]] = (size * rng.choice([-1.0, 1.0], n))[diag]
    _, kind = views(rng, n, tree, zero)
    back = np.where(kind == 0, rng.uniform(0.5, 3.0, n), np.where(kind == 1, 40.0, 2.0 ** 22)) * tree.scale / size
    faces = np.zeros((n, 6), dtype=bool)
    faces[rows, k] = faces[rows, k + 3] = ~diag
    faces[rows[diag], (k + 3 * sk)[diag]] = True
    faces[rows[diag], (j + 3 * sj)[diag]] = True
    if zero:
        o, d = np.zeros((n, 3)), pt.copy()
    else:
        o = pt - d * back[:, None]
    d = rescale(rng, d)
    te, _, tx = slab_entry(lo, hi, o, d)
    base = np.where(te > 0.0, te, tx)
    base = np.where(np.isfinite(base) & (base > 0.0), base, 1.0)
    t_max = np.where(sub == 1, base * (1.0 - 10.0 ** rng.uniform(-6.0, -1.0, n)), PT_MAX_FINITE)
    return Family(o, d, leaf, t_max, faces)


def fam_directions(rng, tree, n, zero):
    """a component of +-0.0, |1/d| up to 1e18, a subnormal component (its reciprocal is infinite: the exact slab test); the origin's
    coordinate on that axis inside the box's slab, on its face, or +-4 ulps off it -- the ray does not move along that axis"""
    leaf, lo, hi = pick(rng, tree, n)
    rows = np.arange(n)
    pt, faces = feature_points(rng, lo, hi, rng.integers(0, 3, n))
    inner = rng.integers(0, 2, n) == 0
    pt = np.where(inner[:, None], lo + (hi - lo) * rng.uniform(0.0, 1.0, (n, 3)), pt)
    faces[inner] = False
    o, _ = views(rng, n, tree, zero)
    ax = rng.integers(0, 3, n)
    if not zero:
        where = rng.integers(0, 3, n)
        side = rng.integers(0, 2, n)
        coord = np.where(side == 1, hi[rows, ax], lo[rows, ax])
        o[rows, ax] = np.where(where == 0, lo[rows, ax] + (hi - lo)[rows, ax] * rng.uniform(0.0, 1.0, n),
                               np.where(where == 1, coord, coord + np.abs(coord) * rng.integers(-4, 5, n) * U32))
        faces[rows, ax] |= (where > 0) & (side == 0)
        faces[rows, ax + 3] |= (where > 0) & (side == 1)
    d = rescale(rng, pt - o)
    sub = rng.integers(0, 4 if zero else 3, n)  # (from the origin a quarter keeps its direction: the slab is where it is)
    sign = rng.choice([-1.0, 1.0], n)
    with np.errstate(under="ignore"):
        lead = np.abs(d).max(axis=1)
        special = np.where(sub == 0, sign * 0.0, np.where(sub == 1, sign * lead * 10.0 ** rng.uniform(-18.0, -6.0, n),
                                                          sign * rng.choice([5e-324, 1e-310, 2e-308], n)))
    d[rows, ax] = np.where(sub <= 2, special, d[rows, ax])
    return Family(o, d, leaf, np.full(n, PT_MAX_FINITE), faces)


MAKERS = {"mix": fam_mix, "edges": fam_edges, "t_max": fam_t_max, "origin": fam_origin, "thin": fam_thin, "directions": fam_directions}


class Triples:
    """.o .d .node .t_max, .family (index into FAMILIES), .aimed_leaf (the triple's node is the leaf its family aimed at, or -- mix --
    a leaf; the others are inner nodes)"""


def make_triples(tree, seed, per_family, zero=False):
    rng = np.random.default_rng(seed)
    parts = []
    for f, name in enumerate(FAMILIES):
        fam = MAKERS[name](rng, tree, per_family, zero)
        n = len(fam.node)
        idx, node = [np.arange(n)], [fam.node]
        if fam.faces is not None and len(tree.bbox) > 1:  # every ancestor whose box shares the targeted face coordinates
            own = tree.bbox[fam.node]
            cur, alive = fam.node.copy(), fam.faces.any(axis=1)
            while alive.any():
                par = tree.parent[cur]
                alive &= par >= 0
                shares = ((tree.bbox[np.maximum(par, 0)] == own) | ~fam.faces).all(axis=1)
                alive &= shares
                idx.append(np.nonzero(alive)[0])
                node.append(par[alive])
                cur = np.where(alive, par, cur)
        idx, node = np.concatenate(idx), np.concatenate(node)
        parts.append((fam.o[idx], fam.d[idx], node, fam.t_max[idx], np.full(len(idx), f)))
    t = Triples()
    t.o, t.d = (np.ascontiguousarray(np.concatenate([p[k] for p in parts])) for k in (0, 1))
    t.node = np.concatenate([p[2] for p in parts]).astype(np.int32)
    t.t_max = np.ascontiguousarray(np.concatenate([p[3] for p in parts]))
    t.family = np.concatenate([p[4] for p in parts])
    t.aimed_leaf = tree.leaf[t.node]
    assert np.isfinite(t.t_max).all() and (t.t_max >= 0.0).all()
    return t
