"""Degenerate inputs for the BVH builders, shared by tests/test_bvh_families.py (host builder against the oracle, no GPU)
and tests/test_gpu_bvh_families.py (GPU builder against the host builder).

Random meshes never reach the rules the GPU builder (csrc/bvh_build_gpu.inc) restates by hand: equal costs along an axis
and between axes, an axis without extent, a total box without area (every cost NaN), thousands of coincident centroids in
the tiled path, segment sizes on both sides of every size class (64 | 65 one wave, 2047 | 2048 private bins, 8191 | 8192
tiles, multiples of the 2048-element tile), signed zeros.  Every family is deterministic (fixed seeds) and is built through
make_desc of test_gpu_edge_cases: Array leaves, length_cutoff 4 and 32 bins unless its entry says otherwise.

FAMILIES maps a name to a function returning (desc, keepalive).  MAX_DEPTH is a condition on every family, checked on
the host-built tree before a device sees the input: nothing in the builder is sized by depth, but no tree deeper than
this has been taken to a device by this suite, and this module is not the place to start.
"""
import numpy as np

from test_gpu_edge_cases import make_desc

MAX_DEPTH = 64


def _desc(spheres=(), tris=(), leaf_kind=1, cutoff=4, num_bins=32):
    from path_tracer_ocaml_amd import abi
    sph = [(float(s[0]), float(s[1]), float(s[2]), float(s[3]), k % 3) for k, s in enumerate(spheres)]
    d, keep = make_desc(abi, spheres=sph, tris=list(tris), leaf_kind=leaf_kind, cutoff=cutoff)
    d.num_bins = num_bins
    return d, keep


def soup(n, seed, scale=1.0, centre=(0.0, 0.0, -5.0)):
    """n spheres, centres uniform in a cube of half-width `scale` about `centre`, radii 0.01 .. 0.05 of it: (n, 4)."""
    rng = np.random.default_rng(seed)
    c = np.array(centre) + rng.uniform(-1, 1, (n, 3)) * scale
    r = rng.uniform(0.01, 0.05, n) * scale
    return np.column_stack([c, r])


# ---------------------------------------------------------------- size edges
SIZE_EDGES = (1, 4, 5, 64, 65, 2047, 2048, 2049, 4095, 4096, 8191, 8192, 8193, 10240, 10241, 20000)
SIMD_SIZE_EDGES = (8192, 10241)  # Simd leaves, cutoff 16: the pad4 path of k_fin_sizes


def size_edge(n, leaf_kind=1, cutoff=4):
    return _desc(soup(n, 1000 + n), leaf_kind=leaf_kind, cutoff=cutoff)


# ---------------------------------------------------------------- skewed
def skewed():
    """12000 spheres, 11900 of them in a cluster 1e-3 of the scene wide: a tiled segment hands out a tiled, a workgroup and
    a wave child in one level."""
    s = soup(12000, 11)
    s[:11900, :3] = s[:11900, :3] * 1e-3 + np.array([0.9, 0.9, -4.1])
    s[:11900, 3] *= 1e-3
    return _desc(s)


# ---------------------------------------------------------------- duplicates
def duplicates(leaf_kind=1, cutoff=4):
    """700 distinct spheres, each 13 times: 13 coincident centroids cannot be split, whatever the cutoff."""
    return _desc(np.repeat(soup(700, 12), 13, axis=0), leaf_kind=leaf_kind, cutoff=cutoff)


COINCIDENT_N = 9000


def coincident():
    """9000 identical spheres: no axis has a finite scale, so the root is one 9000-element leaf, decided by k_big_split
    and written by one thread of k_fin_emit."""
    return _desc(np.tile(np.array([[0.0, 0.0, -5.0, 1.0]]), (COINCIDENT_N, 1)))


def concentric():
    """9000 spheres about one centre with different radii: the same centroid, different boxes."""
    c = np.tile(np.array([[0.0, 0.0, -5.0, 1.0]]), (9000, 1))
    c[:, 3] = np.random.default_rng(13).uniform(0.1, 1.0, 9000)
    return _desc(c)


# ---------------------------------------------------------------- zero-range axes
def line_x():
    s = soup(9000, 14)
    s[:, 1] = 0.25
    s[:, 2] = -5.0
    return _desc(s)


def plane_xy():
    s = soup(9000, 15)
    s[:, 2] = -5.0
    return _desc(s)


# ---------------------------------------------------------------- exact ties
def lattice_points(nx, ny, nz):
    """(n, 4): spheres of radius 0.25 on an integer lattice.  Every bound is a multiple of 0.25 below 2^6, so box areas,
    their products with element counts and the sums of two of them are exact in binary64, fused or not."""
    return np.array([[x, y, -5.0 - z, 0.25] for x in range(nx) for y in range(ny) for z in range(nz)], float)


LATTICES = {"lattice-21x21x21": (21, 21, 21), "lattice-32x32x16": (32, 32, 16)}


def lattice(name):
    return _desc(lattice_points(*LATTICES[name]))


# ---------------------------------------------------------------- zero-area boxes
def flat_triangles():
    """5000 triangles in the plane z = -5"""
    rng = np.random.default_rng(16)
    tris = []
    for _ in range(5000):
        c = rng.uniform(-1, 1, 2)
        p = c + rng.uniform(-0.05, 0.05, (3, 2))
        tris.append(((p[0, 0], p[0, 1], -5.0), (p[1, 0], p[1, 1], -5.0), (p[2, 0], p[2, 1], -5.0), 0))
    return _desc(tris=tris)


def point_triangles():
    """5000 triangles whose three vertices coincide, in the plane z = -5: every element box is a point"""
    rng = np.random.default_rng(17)
    tris = []
    for _ in range(5000):
        p = (*rng.uniform(-1, 1, 2), -5.0)
        tris.append((p, p, p, 0))
    return _desc(tris=tris)


COLLINEAR_N = 150  # do not grow: 300 gives depth 71, 5000 depth 140 (MAX_DEPTH)


def collinear_vertices():
    rng = np.random.default_rng(18)
    x = np.sort(rng.uniform(-1, 1, (COLLINEAR_N, 3)), axis=1)
    return x


def collinear_triangles():
    """150 triangles whose vertices all lie on one line along x: the box of any subset has no area, so every candidate
    cost is 0.25 + 0 / 0 = NaN and the NaN order of Float.compare decides every split."""
    tris = [((x[0], 0.5, -5.0), (x[1], 0.5, -5.0), (x[2], 0.5, -5.0), 0) for x in collinear_vertices()]
    return _desc(tris=tris)


# ---------------------------------------------------------------- scales
def scale_offset_2p40():
    """width 1, centred 2^40 away: the centroids quantise to multiples of 2^-13"""
    return _desc(soup(9000, 19, 1.0, (2.0 ** 40, 0.0, -5.0)))


def scale_2m20_at_1():
    return _desc(soup(9000, 20, 2.0 ** -20, (1.0, 1.0, -5.0)))


def scale_2p100():
    return _desc(soup(9000, 21, 2.0 ** 100))


# ---------------------------------------------------------------- geometric progression
def geometric():
    """x = 2^-(k mod 48): each split cuts off the upper half of what is left, a chain as deep as the progression is long"""
    k = np.arange(9000)
    e = 2.0 ** -(k % 48)
    return _desc(np.column_stack([e * (1 + k // 48 * 1e-3), np.zeros(9000), -5.0 * np.ones(9000), 1e-3 * e]))


# ---------------------------------------------------------------- signed zeros
def signed_zero_triangles(variant):
    """4200 triangles on a 70 x 60 grid whose vertex a has y = +-0.0, the minimum of its triangle.
    "mixed": the sign drawn at random; "negative": every zero -0.0; "mirror": the mixed scene with y negated, so that the
    maxima carry the zeros."""
    rng = np.random.default_rng(22)
    tris = []
    for k in range(4200):
        x, zc = float(k % 70) + 1.0, float(k // 70)
        neg = bool(rng.integers(0, 2))
        by = 1.0 + rng.random()
        ay = -0.0 if (neg or variant == "negative") else 0.0
        t = [(x, ay, -5.0 - zc), (x + 0.5, by, -5.0 - zc), (x + 0.25, 0.5, -4.5 - zc)]
        if variant == "mirror":
            t = [(p[0], -p[1], p[2]) for p in t]
        tris.append((*t, 0))
    return _desc(tris=tris)


def alternating_zero_triangles(order):
    """40 triangles in a row along x whose minimum y alternates between +0.0 and -0.0, beginning with order[0] (1 = -0.0).
    Float.min keeps its SECOND argument on a tie, so which zero a union keeps depends on the order of the slice."""
    rng = np.random.default_rng(3)
    tris = []
    for k in range(40):
        x = float(k) + 1.0
        ay = -0.0 if order[k % len(order)] else 0.0
        tris.append(((x, ay, -5.0), (x + 0.5, 1.0 + rng.random(), -5.0), (x + 0.25, 0.5, -4.0 - rng.random()), 0))
    return _desc(tris=tris)


# ---------------------------------------------------------------- bin counts
BIN_COUNTS = (4, 64, 65)  # 2 is refused by the descriptor check; 65 is more than the GPU builder's 64


def bins_soup(num_bins):
    return _desc(soup(9000, 23), num_bins=num_bins)


# ---------------------------------------------------------------- the registry
FAMILIES = {}
for _n in SIZE_EDGES:
    FAMILIES[f"soup-{_n}"] = (lambda n=_n: size_edge(n))
for _n in SIMD_SIZE_EDGES:
    FAMILIES[f"soup-{_n}-simd16"] = (lambda n=_n: size_edge(n, leaf_kind=0, cutoff=16))
FAMILIES.update({
    "skewed-12000": skewed,
    "duplicates-700x13": duplicates,
    "duplicates-700x13-simd16": lambda: duplicates(leaf_kind=0, cutoff=16),
    "coincident-9000": coincident,
    "concentric-9000": concentric,
    "line-x-9000": line_x,
    "plane-xy-9000": plane_xy,
    "lattice-21x21x21": lambda: lattice("lattice-21x21x21"),
    "lattice-32x32x16": lambda: lattice("lattice-32x32x16"),
    "flat-triangles-5000": flat_triangles,
    "point-triangles-5000": point_triangles,
    "collinear-triangles-150": collinear_triangles,
    "offset-2p40": scale_offset_2p40,
    "scale-2m20-at-1": scale_2m20_at_1,
    "scale-2p100": scale_2p100,
    "geometric-48": geometric,
    "signed-zero-mixed": lambda: signed_zero_triangles("mixed"),
    "signed-zero-negative": lambda: signed_zero_triangles("negative"),
    "signed-zero-mirror": lambda: signed_zero_triangles("mirror"),
})
for _b in BIN_COUNTS:
    FAMILIES[f"soup-9000-bins{_b}"] = (lambda b=_b: bins_soup(b))

# what the GPU builder refuses: more bins than it has, and bound columns that hold both zeros (DESIGN F3)
GPU_REFUSED = {"soup-9000-bins65": "num_bins", "signed-zero-mixed": "zero", "signed-zero-mirror": "zero"}
GPU_FAMILIES = [name for name in FAMILIES if name not in GPU_REFUSED]


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def same_tree(a, b):
    """Messages for every part of two tree() results that differs, boxes compared as bits"""
    msgs = []
    for what, x, y in zip(("node boxes", "node info", "leaf element order"), a, b):
        if x.shape != y.shape:
            msgs.append(f"{what}: shapes {x.shape} and {y.shape}")
        elif what == "node boxes":
            if not np.array_equal(bits(x), bits(y)):
                bad = np.nonzero((bits(x) != bits(y)).reshape(len(x), -1).any(1))[0]
                msgs.append(f"{what} differ in {len(bad)} nodes, first {int(bad[0])}: {x[bad[0]].tolist()} and {y[bad[0]].tolist()}")
        elif not np.array_equal(x, y):
            msgs.append(f"{what} differ in {int((x != y).reshape(len(x), -1).any(1).sum())} rows")
    return msgs


STAT_KEYS = ("tree_nodes", "tree_depth", "tree_leaves", "leaf_slots")


def zero_bounds(bbox):
    """(zero-valued bounds, how many of them are -0.0)"""
    z = np.asarray(bbox).reshape(-1)
    z = z[z == 0.0]
    return len(z), int(np.signbit(z).sum())
