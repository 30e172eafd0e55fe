"""The bounce kernels' own tree walks on explicit adversarial rays (ptx_walk_rays, include/ptx.h).

ptx_intersect_rays launches k_trace, whose node loop on an LDS-resident scene is the compiler's; the rays of a render go through other
code: the assembly node loops on the shared and on the per-octant LDS image (PtTraverser::walk_asm, walk_asm_oct), their ORIGIN_ZERO
forms (the camera launch), the divergent loop of the Array_leaf scenes, the camera rays' wave packet, and the tail cut with its
resumption from (node, closest hit).  ptx_walk_rays runs exactly those instantiations on rays handed to it, so the ray families of
tests/test_gpu_fuzz.py, test_gpu_edge_cases.py and test_gpu_exact_geometry.py -- scales from 2^-20 to beyond binary32, origins 2^22
scene widths away, axis-aligned and near-axis directions, box edges grazed within 4 binary32 ulps, coincident spheres, flat boxes --
reach every one of them here.

Bar, everywhere: the hit primitive equal and t equal BIT FOR BIT to the oracle's Scene.intersect on the same rays; on the scenes of
tests/exact_geometry.py also the exact, oracle-independent reference (X.compare empty).  No tolerances.

A PACKET or _ZERO walk takes the origin as (+0, +0, +0).  Their families are ray_mix's directions as they are plus the same kinds of
direction (unnormalised, near-axis with |1/d| up to 1e18, components of +-0.0, box edges grazed within 4 binary32 ulps) aimed from
the origin, and rays aimed inside single spheres down to the smallest, with the soup's centre placed so that the origin is inside
the soup, a few widths outside, and far from it.  The last family seen from afar is what a library with the node's magnitude taken
out of walk_asm_oct's margin fails on (profiles/pr_walk_rays_mutants.txt); without it that library passed this whole file."""
import ctypes as C

import numpy as np
import pytest

import exact_geometry as X
from test_gpu_edge_cases import bits, both, make_desc
from test_gpu_fuzz import SCALES, leaf_boxes, ray_mix, sphere_soup, triangle_soup, wall_soup
from test_gpu_lds_oct import keeps_nodes64, oct_fits, soup_desc

pytestmark = pytest.mark.gpu

ERR_ARG, ERR_STATE = -1, -3


@pytest.fixture(scope="module")
def P():
    import path_tracer_ocaml_amd as P
    assert P.lib().ptx_device_count() >= 1, P.last_error()
    return P


@pytest.fixture(scope="module")
def W():
    """the walks by name, and which of them a leaf kind admits: (on the caller's origins, on +0.0 origins)"""
    from path_tracer_ocaml_amd import abi

    class Walks:
        names = {getattr(abi, k): k[len("PTX_WALK_"):] for k in dir(abi) if k.startswith("PTX_WALK_")}
        SIMD = [abi.PTX_WALK_SHARED_ASM, abi.PTX_WALK_OCT_ASM, abi.PTX_WALK_SHARED_ASM_TAIL, abi.PTX_WALK_OCT_ASM_TAIL]
        SIMD_ZERO = [abi.PTX_WALK_SHARED_ASM_ZERO, abi.PTX_WALK_OCT_ASM_ZERO, abi.PTX_WALK_PACKET]
        ARRAY = [abi.PTX_WALK_SHARED_DIV, abi.PTX_WALK_SHARED_DIV_TAIL]
        ARRAY_ZERO = [abi.PTX_WALK_SHARED_DIV_ZERO, abi.PTX_WALK_PACKET]
        OCT = [abi.PTX_WALK_OCT_ASM, abi.PTX_WALK_OCT_ASM_ZERO, abi.PTX_WALK_OCT_ASM_TAIL]

        @classmethod
        def of(cls, leaf_kind):
            return (cls.SIMD, cls.SIMD_ZERO) if leaf_kind == 0 else (cls.ARRAY, cls.ARRAY_ZERO)
    assert len(Walks.names) == 10
    return Walks


def admits_oct(g_scene):
    """the per-octant image's admit decision as tests/test_gpu_lds_oct.py restates it from the layout's description"""
    st = g_scene.stats()
    n64 = keeps_nodes64(st["tree_nodes"], st["leaf_slots"], st["tree_depth"])
    return n64 is not None and st["tree_nodes"] <= 2047 and oct_fits(st["tree_nodes"], st["leaf_slots"], n64)


def check_walks(W, o_scene, g_scene, walks, o, d):
    """check_rays' comparison (tests/test_gpu_edge_cases.py) for every walk of `walks`: prim equal, t equal bit for bit"""
    o = np.ascontiguousarray(o, dtype=np.float64)
    d = np.ascontiguousarray(d, dtype=np.float64)
    t_c, p_c, _ = o_scene.intersect_rays(o, d)
    if set(walks) & set(W.OCT):  # (what the layout admits must be what the library admits: a refusal would raise)
        assert admits_oct(g_scene)
    for w in walks:
        t_g, p_g = g_scene.walk_rays(w, o, d)
        wrong = np.nonzero((p_g != p_c) | (bits(t_g) != bits(t_c)))[0]
        assert len(wrong) == 0, (W.names[w], len(wrong), [(int(k), int(p_g[k]), int(p_c[k]), float(t_g[k]), float(t_c[k])) for k in wrong[:5]])
    return p_c


def dirs_from_origin(rng, n, scale, centre, boxes, mixed=None, spheres=None):
    """ray_mix's kinds of direction for rays that start at the origin: `mixed` (ray_mix's own directions, kept as they are) for a
    third of the rays; the others aimed at points of the soup, unnormalised; of those a share near-axis (one component scaled by
    1e-18 .. 1e-6), a share with one component exactly +0.0 or -0.0, a share through points on box edges moved by -4 .. +4
    binary32 ulps of their magnitude, and -- given `spheres` (x, y, z, r, ...) -- a share aimed INSIDE a sphere chosen at random,
    the smallest included: seen from afar such a sphere's box is narrower than a binary32 ulp of its distance, the entry and exit
    distances of a ray that hits it coincide in binary32, and only the margin keeps the filter from calling that a miss."""
    kinds = rng.integers(0, 6, n)
    target = centre + rng.uniform(-1.0, 1.0, (n, 3)) * scale
    d = target.copy()
    if spheres is not None:
        aimed = kinds == 0
        sp = np.array([s_[:4] for s_ in spheres], dtype=np.float64)[rng.integers(0, len(spheres), aimed.sum())]
        d[aimed] = sp[:, :3] + rng.uniform(-0.5, 0.5, (aimed.sum(), 3)) * sp[:, 3:]
    graze = kinds == 5
    k = int(graze.sum())
    bx = boxes[rng.integers(0, len(boxes), k)]
    a1 = rng.integers(0, 3, k)
    a2 = (a1 + 1 + rng.integers(0, 2, k)) % 3
    a3 = 3 - a1 - a2
    rows = np.arange(k)
    pt = np.zeros((k, 3))
    pt[rows, a1] = bx[rows, a1 + 3 * rng.integers(0, 2, k)]
    pt[rows, a2] = bx[rows, a2 + 3 * rng.integers(0, 2, k)]
    pt[rows, a3] = bx[rows, a3] + (bx[rows, a3 + 3] - bx[rows, a3]) * rng.uniform(0.0, 1.0, k)
    pt += np.abs(pt) * rng.integers(-4, 5, (k, 3)) * 2.0 ** -24
    d[graze] = pt
    with np.errstate(over="ignore"):
        d *= 10.0 ** rng.uniform(-3.0, 3.0, (n, 1))
    ax = rng.integers(0, 3, n)
    near_axis = kinds == 3
    d[near_axis, ax[near_axis]] *= 10.0 ** rng.uniform(-18.0, -6.0, near_axis.sum())
    on_axis = kinds == 4
    d[on_axis, ax[on_axis]] = np.where(rng.integers(0, 2, on_axis.sum()) == 0, 0.0, -0.0)
    two = on_axis & (rng.integers(0, 3, n) == 0)  # ... and some along an axis exactly: two components of +-0.0
    d[two, (ax[two] + 1) % 3] = np.where(rng.integers(0, 2, two.sum()) == 0, 0.0, -0.0)
    if mixed is not None:
        d[::3] = mixed[: len(d[::3])]
    return d


def simd_soup(P, oracle, seed, scale):
    """test_sphere_soup_simd_leaf's scene and rays"""
    from path_tracer_ocaml_amd import abi
    rng = np.random.default_rng(1000 + seed)
    centre = rng.uniform(-1.0, 1.0, 3) * scale * (50.0 if seed >= 7 else 3.0)
    sph = sphere_soup(rng, 300, scale, centre)
    d, keep = make_desc(abi, spheres=sph, leaf_kind=0, cutoff=16)
    o_scene, g_scene = both(P, oracle, d, keep)
    g_scene.spheres = np.array([s[:4] for s in sph])
    assert g_scene.stats()["traversal_in_lds"]
    o, dr = ray_mix(rng, 30000, scale, centre, leaf_boxes(g_scene))
    return o_scene, g_scene, o, dr


SOUPS = [(s, sc) for s, sc in enumerate(SCALES)] + [(7, 1.0), (8, 2.0 ** 21), (9, 2.0 ** -20)]


# ---- 1. sphere soups through both assembly loops, plain and with the tail cut
@pytest.mark.parametrize("seed,scale", SOUPS)
def test_sphere_soups_through_both_assembly_loops(P, W, oracle, seed, scale):
    o_scene, g_scene, o, dr = simd_soup(P, oracle, seed, scale)
    prims = check_walks(W, o_scene, g_scene, W.SIMD, o, dr)
    assert (prims >= 0).sum() > 300 and (prims < 0).sum() > 300
    # the same filter arithmetic where it can count (the assembly loops cannot): the grazing rays graze
    assert g_scene.intersect_rays(o, dr)[2]["filter_undecided"] > 0
    g_scene.close()


# ---- 2. the origin-zero forms and the packet walk
PLACES = {"inside": 0.3, "outside": 4.0, "far": 1000.0}  # |centre| in soup half-widths


@pytest.mark.parametrize("place", list(PLACES))
@pytest.mark.parametrize("seed,scale", [(s, sc) for s, sc in enumerate(SCALES)])
def test_origin_zero_forms_and_the_packet(P, W, oracle, seed, scale, place):
    from path_tracer_ocaml_amd import abi
    rng = np.random.default_rng(2000 + seed)
    centre = np.array([0.3, -0.2, -0.9]) / np.linalg.norm([0.3, -0.2, -0.9]) * scale * PLACES[place]
    sph = sphere_soup(rng, 300, scale, centre)
    d, keep = make_desc(abi, spheres=sph, leaf_kind=0, cutoff=16)
    o_scene, g_scene = both(P, oracle, d, keep)
    assert g_scene.stats()["traversal_in_lds"]
    boxes = leaf_boxes(g_scene)
    _, mixed = ray_mix(rng, 20000, scale, centre, boxes)
    dr = dirs_from_origin(rng, 20000, scale, centre, boxes, mixed, sph)
    assert ((dr == 0.0).sum(axis=1) >= 1).sum() > 1000 and ((dr == 0.0).sum(axis=1) == 2).sum() > 100
    nz = np.abs(dr[(dr != 0.0).all(axis=1)])
    assert (nz.max(axis=1) / nz.min(axis=1) > 1e9).sum() > 300  # near-axis: one reciprocal dwarfs the others
    o = np.zeros_like(dr)
    prims = check_walks(W, o_scene, g_scene, W.SIMD_ZERO + W.SIMD, o, dr)
    assert (prims >= 0).sum() > 1500 and (prims < 0).sum() > 300  # (the rays aimed inside a sphere hit: a ninth of all)
    assert g_scene.intersect_rays(o, dr)[2]["filter_undecided"] > 0
    g_scene.close()


# ---- 3. Array_leaf: the divergent loop, its tail cut, the packet
@pytest.mark.parametrize("seed,scale", [(20, 2.0 ** -12), (21, 1.0), (22, 2.0 ** 14), (23, 2.0 ** 21)])
def test_mixed_soups_array_leaf(P, W, oracle, seed, scale):
    """test_mixed_soup_array_leaf_lds' scenes and rays, then the same soup seen from the origin"""
    from path_tracer_ocaml_amd import abi
    rng = np.random.default_rng(seed)
    centre = rng.uniform(-1.0, 1.0, 3) * scale * 3.0
    sph = sphere_soup(rng, 60, scale, centre, 4.0)
    d, keep = make_desc(abi, spheres=sph, tris=triangle_soup(rng, 80, scale, centre), leaf_kind=1, cutoff=3)
    o_scene, g_scene = both(P, oracle, d, keep)
    assert g_scene.stats()["traversal_in_lds"]
    boxes = leaf_boxes(g_scene)
    o, dr = ray_mix(rng, 20000, scale, centre, boxes)
    prims = check_walks(W, o_scene, g_scene, W.ARRAY, o, dr)
    assert (prims < 0).sum() > 100
    if scale >= 1.0:
        assert (prims >= 0).sum() > 100
    assert g_scene.intersect_rays(o, dr)[2]["filter_undecided"] > 0
    dz = dirs_from_origin(rng, 10000, scale, centre, boxes, dr, sph)
    prims = check_walks(W, o_scene, g_scene, W.ARRAY_ZERO + W.ARRAY, np.zeros_like(dz), dz)
    assert (prims < 0).sum() > 100 and (prims >= 0).sum() > 500  # (the rays aimed inside a sphere hit, whatever the scale)
    g_scene.close()


# ---- 4. magnitude edges
@pytest.mark.parametrize("leaf_kind,cutoff,scale", [(0, 16, 1e39), (1, 4, 1e39), (0, 16, 3e37), (1, 4, 1e300)])
def test_bounds_beyond_binary32_range(P, W, oracle, leaf_kind, cutoff, scale):
    """test_bounds_beyond_binary32_range's scenes: every visit leaves the assembly loops through their undecided exit"""
    from path_tracer_ocaml_amd import abi
    rng = np.random.default_rng(77)
    centre = np.array([0.3, -0.2, -4.0]) * scale
    sph = sphere_soup(rng, 120, scale, centre, 3.0)
    d, keep = make_desc(abi, spheres=sph, leaf_kind=leaf_kind, cutoff=cutoff)
    o_scene, g_scene = both(P, oracle, d, keep)
    boxes = leaf_boxes(g_scene)
    o, dr = ray_mix(rng, 8000, scale, centre, boxes)
    o[::2] = 0.0
    here, zero = W.of(leaf_kind)
    with np.errstate(over="ignore", invalid="ignore"):
        prims = check_walks(W, o_scene, g_scene, here, o, dr)
        if scale < 1e100:
            assert (prims >= 0).sum() > 100
        dz = dirs_from_origin(rng, 8000, scale, centre, boxes, dr, sph)
        prims = check_walks(W, o_scene, g_scene, zero + here, np.zeros_like(dz), dz)
        if scale < 1e100:
            assert (prims >= 0).sum() > 100
    g_scene.close()


def test_every_test_undecided_when_margin_is_everything(P, W, oracle):
    """the lattice of test_gpu_fuzz.py's test of that name, seen edge-on: rays inside shared box planes, exactly and a few ulps off"""
    from path_tracer_ocaml_amd import abi
    rng = np.random.default_rng(5)
    spheres = [(float(x), float(y), -8.0, 0.5, 0) for x in range(-6, 7) for y in range(-6, 7)]
    d, keep = make_desc(abi, spheres=spheres, leaf_kind=0, cutoff=16)
    o_scene, g_scene = both(P, oracle, d, keep)
    n = 6000
    o = np.zeros((n, 3))
    o[:, 0] = rng.integers(-6, 7, n) + 0.5 * rng.choice([-1.0, 1.0], n)
    o[:, 1] = rng.integers(-6, 7, n) + 0.5 * rng.choice([-1.0, 1.0], n)
    o[:, :2] += np.abs(o[:, :2]) * rng.integers(-2, 3, (n, 2)) * 2.0 ** -24
    dr = np.tile([0.0, 0.0, -1.0], (n, 1))
    dr[: n // 2, 0] = rng.normal(size=n // 2) * 1e-9
    check_walks(W, o_scene, g_scene, W.SIMD, o, dr)
    assert g_scene.intersect_rays(o, dr)[2]["filter_undecided"] > n // 4
    # from the origin: the planes x = 0 +- 0.5 ... are not through it, the planes of the lattice's symmetry are -- directions inside
    # x = 0 and y = 0 (a component of +-0.0) and a few ulps off them, towards every column and row of the lattice
    dz = np.zeros((n, 3))
    dz[:, 2] = -8.0
    dz[:, 0] = rng.integers(-6, 7, n) + 0.5 * rng.choice([-1.0, 0.0, 1.0], n)
    dz[:, 1] = rng.integers(-6, 7, n) + 0.5 * rng.choice([-1.0, 0.0, 1.0], n)
    dz[: n // 2, :2] += np.abs(dz[: n // 2, :2]) * rng.integers(-2, 3, (n // 2, 2)) * 2.0 ** -24
    prims = check_walks(W, o_scene, g_scene, W.SIMD_ZERO + W.SIMD, np.zeros_like(dz), dz)
    assert (prims >= 0).sum() > 300 and (prims < 0).sum() > 300
    g_scene.close()


@pytest.mark.parametrize("seed,scale,cutoff", [(50, 1.0, 4), (51, 2.0 ** -11, 2), (52, 2.0 ** 18, 1), (53, 1.0, 1)])
def test_flat_boxes_axis_aligned_walls(P, W, oracle, seed, scale, cutoff):
    """test_flat_boxes_axis_aligned_walls' scenes and rays: boxes of zero thickness, where near equals far"""
    from path_tracer_ocaml_amd import abi
    rng = np.random.default_rng(1000 + seed)
    centre = rng.uniform(-1.0, 1.0, 3) * scale * 3.0
    d, keep = make_desc(abi, tris=wall_soup(rng, 200, scale, centre), leaf_kind=1, cutoff=cutoff)
    o_scene, g_scene = both(P, oracle, d, keep)
    assert g_scene.stats()["traversal_in_lds"]
    boxes = leaf_boxes(g_scene)
    flat = boxes[(boxes[:, :3] == boxes[:, 3:]).any(axis=1)]
    assert len(flat) > 20, "the scene was meant to have flat boxes"
    o, dr = ray_mix(rng, 30000, scale, centre, boxes)
    k = 3000
    bx = flat[rng.integers(0, len(flat), k)]
    ax = np.argmax(bx[:, :3] == bx[:, 3:], axis=1)
    o[:k, :] = centre + rng.uniform(-1.0, 1.0, (k, 3)) * scale
    o[np.arange(k), ax] = bx[np.arange(k), ax]
    dr[:k] = rng.normal(size=(k, 3))
    dr[np.arange(k), ax] = 0.0
    prims = check_walks(W, o_scene, g_scene, W.ARRAY, o, dr)
    assert (prims >= 0).sum() > 300 and (prims < 0).sum() > 300
    dz = dirs_from_origin(rng, 10000, scale, centre, flat, dr)  # the grazed edges: the flat boxes'
    prims = check_walks(W, o_scene, g_scene, W.ARRAY_ZERO + W.ARRAY, np.zeros_like(dz), dz)
    assert (prims < 0).sum() > 100
    if scale >= 1.0:  # |det| < 1e-6 rejects the triangles of a tiny scene for directions of the scene's own size (triangle.ml:83)
        assert (prims >= 0).sum() > 100
    g_scene.close()


# ---- 5. the exact, oracle-independent reference
LDS_SCENES = [n for n in X.SCENES if n != "ganesha_150k"]


@pytest.mark.parametrize("name", LDS_SCENES)
def test_walks_equal_the_exact_reference(P, W, oracle, name):
    """Every walk the scene admits (a scene walked from HBM / L2 admits none: the refusal is asserted) on X.make_rays' rays: X.compare and X.check_floors empty (the floors of tests/exact_geometry.py, as
    they are).  The PACKET and _ZERO walks take the same directions from the origin, against a second exact reference of those rays:
    X.compare empty (the floors are statements about make_rays' set, whose aim points the moved origin gives up)."""
    from path_tracer_ocaml_amd import abi
    ptr, keep = X.scene_desc(name, oracle, abi)
    geo = X.Geometry(ptr)
    O, D = X.make_rays(geo, 1500, seed=sum(map(ord, name)))
    res = X.Reference(geo).closest(O, D)
    Z = np.zeros_like(O)
    res0 = X.Reference(geo).closest(Z, D)
    g = P.Scene(ptr, 0, keepalive=keep)
    o_scene = oracle.Scene(ptr, keep)
    try:
        leaf_kind = int(ptr.contents.leaf_kind)
        here, zero = W.of(leaf_kind)
        if not g.stats()["traversal_in_lds"]:  # (ganesha_3k: walked from HBM / L2 -- no walk of these is the scene's)
            for w in sorted(W.names):
                with pytest.raises(P.PtxError, match="HBM"):
                    g.walk_rays(w, Z, D)
            here = zero = []
        elif leaf_kind == 0 and not admits_oct(g):
            for w in W.OCT:
                with pytest.raises(P.PtxError, match="per-octant"):
                    g.walk_rays(w, Z, D)
            here, zero = [w for w in here if w not in W.OCT], [w for w in zero if w not in W.OCT]
        for walks, o, r in ((here, O, res), (zero, Z, res0)):
            t_c, p_c, _ = o_scene.intersect_rays(o, D)
            for w in walks:
                t, prim = g.walk_rays(w, o, D)
                assert np.array_equal(prim, p_c) and np.array_equal(bits(t), bits(t_c)), W.names[w]
                bad = X.compare(r, prim, t)
                assert not bad, W.names[w] + "\n" + "\n".join(bad)
                if r is res:
                    floors = X.check_floors(name, r.summary(t))
                    assert not floors, "\n".join(floors)
        assert res0.summary()["robust"] > 0.5 * len(D)
    finally:
        g.close()


# ---- 6. wave shape
@pytest.fixture(scope="module")
def one_soup(P, oracle):
    o_scene, g_scene, o, dr = simd_soup(P, oracle, 2, 1.0)
    yield o_scene, g_scene, o, dr
    g_scene.close()


@pytest.mark.parametrize("n", [1, 63, 64, 65, 4097])
def test_partial_and_ragged_chunks(P, W, one_soup, n):
    """a last chunk with one live lane, full chunks, a ragged tail"""
    o_scene, g_scene, o, dr = one_soup
    hits = np.nonzero(o_scene.intersect_rays(o, dr)[1] >= 0)[0]
    first = hits[0] if n == 1 else 0  # (the one ray: one that walks to a hit)
    check_walks(W, o_scene, g_scene, W.SIMD, o[first:first + n], dr[first:first + n])
    check_walks(W, o_scene, g_scene, W.SIMD_ZERO + W.SIMD, np.zeros((n, 3)), dr[first:first + n])


def test_few_deep_rays_among_lanes_that_leave_at_the_root(P, W, one_soup):
    """60 of every 64 consecutive rays miss the root box (aimed away from the scene), 4 go deep: once a lane has left, fewer than
    PT_WALK_MIN are walking -- that exit of both assembly loops -- and fewer than PT_TAIL_CUT, the tail cut.  The same rays in
    shuffled order: a ray's result does not depend on which rays share its wave."""
    o_scene, g_scene, o, dr = one_soup
    rng = np.random.default_rng(6)
    bbox = leaf_boxes(g_scene)[0]
    mid, half = (bbox[:3] + bbox[3:]) / 2, (bbox[3:] - bbox[:3]).max() / 2
    n = 64 * 64
    oo = mid + rng.normal(size=(n, 3)) / np.sqrt(3.0) * half * 6.0
    oo += np.sign(oo - mid) * half * 1.5  # outside the root box on every axis
    dd = (oo - mid) * 10.0 ** rng.uniform(-2.0, 2.0, (n, 1))  # away
    deep = np.zeros(n, bool)
    for c in range(64):
        deep[64 * c + rng.choice(64, 4, replace=False)] = True
    big = g_scene.spheres[np.argsort(g_scene.spheres[:, 3])[-40:]]  # the 40 largest spheres: aimed inside one, a ray walks down to it
    aim = big[rng.integers(0, len(big), deep.sum())]
    aim = aim[:, :3] + rng.uniform(-0.5, 0.5, (deep.sum(), 3)) * aim[:, 3:]
    dd[deep] = aim - oo[deep]
    t_c, p_c, st = o_scene.intersect_rays(oo, dd)
    assert (p_c[~deep] < 0).all() and (p_c[deep] >= 0).all()
    check_walks(W, o_scene, g_scene, W.SIMD, oo, dd)
    perm = rng.permutation(n)
    for w in W.SIMD:
        t_a, p_a = g_scene.walk_rays(w, oo, dd)
        t_b, p_b = g_scene.walk_rays(w, oo[perm], dd[perm])
        assert np.array_equal(p_b, p_a[perm]) and np.array_equal(bits(t_b), bits(t_a[perm])), W.names[w]
    # from the origin: 60 of 64 directions away from the soup, 4 at it
    dz = -(mid + rng.uniform(-1.0, 1.0, (n, 3)) * half)
    dz[deep] = aim
    p0 = check_walks(W, o_scene, g_scene, W.SIMD_ZERO + W.SIMD, np.zeros_like(dz), dz)
    assert (p0[~deep] < 0).all() and (p0[deep] >= 0).all()


def test_sixty_four_copies_of_one_ray(P, W, one_soup):
    o_scene, g_scene, o, dr = one_soup
    p_c = o_scene.intersect_rays(o, dr)[1]
    for k in (np.nonzero(p_c >= 0)[0][0], np.nonzero(p_c < 0)[0][0]):
        prims = check_walks(W, o_scene, g_scene, W.SIMD, np.tile(o[k], (64, 1)), np.tile(dr[k], (64, 1)))
        assert (prims == p_c[k]).all()
        check_walks(W, o_scene, g_scene, W.SIMD_ZERO, np.zeros((64, 3)), np.tile(dr[k], (64, 1)))


# ---- 7. ties and degenerate packets
def test_coincident_spheres_tie_rule_and_unsplittable_leaf(P, W, oracle):
    """one leaf holding seven identical spheres: equal t, the later element wins; a tree of one node"""
    from path_tracer_ocaml_amd import abi
    spheres = [(0.0, 0.0, -5.0, 1.0, k % 3) for k in range(7)]
    dirs = np.array([[x, y, -1.0] for x in np.linspace(-0.3, 0.3, 15) for y in np.linspace(-0.3, 0.3, 15)])
    for leaf_kind, cutoff in ((0, 16), (1, 4)):
        d, keep = make_desc(abi, spheres=spheres, leaf_kind=leaf_kind, cutoff=cutoff)
        o_scene, g_scene = both(P, oracle, d, keep)
        assert g_scene.stats()["tree_nodes"] == 1
        here, zero = W.of(leaf_kind)
        prims = check_walks(W, o_scene, g_scene, zero + here, np.zeros_like(dirs), dirs)
        assert set(prims.tolist()) == {-1, 6}
        g_scene.close()


def test_rays_from_inside_spheres_and_tiny_scenes(P, W, oracle):
    from path_tracer_ocaml_amd import abi
    rng = np.random.default_rng(2)
    dirs = rng.normal(size=(5000, 3))
    off = np.tile([0.1, -0.2, 0.3], (5000, 1))
    for spheres in ([(0.0, 0.0, 0.0, 3.0, 2), (0.5, 0.2, -1.0, 0.4, 1)], [(0.5, 0.2, -1.0, 0.4, 1)]):  # two spheres; one
        d, keep = make_desc(abi, spheres=spheres, leaf_kind=0, cutoff=16)
        o_scene, g_scene = both(P, oracle, d, keep)
        prims = check_walks(W, o_scene, g_scene, W.SIMD_ZERO + W.SIMD, np.zeros((5000, 3)), dirs)
        assert 0.01 < (prims >= 0).mean() < 1.0
        check_walks(W, o_scene, g_scene, W.SIMD, off, dirs)
        g_scene.close()
    # a scene without a tree (n_nodes == 0) cannot be made: the library refuses an empty list of shapes, as the reference does
    d, keep = make_desc(abi, leaf_kind=0, cutoff=16)
    with pytest.raises(P.PtxError, match="non-empty"):
        P.Scene(d, 0, keepalive=keep)


# ---- 8. refusals
def raw_call(P, g, walk, o, d, n=None, null=()):
    o = np.ascontiguousarray(o, dtype=np.float64)
    d = np.ascontiguousarray(d, dtype=np.float64)
    n = len(o) if n is None else n
    t, prim = np.full(max(n, 1), -7.0), np.full(max(n, 1), -7, dtype=np.int32)
    dp, ip = P.abi.c_double_p, P.abi.c_int32_p
    args = [o.ctypes.data_as(dp), d.ctypes.data_as(dp), t.ctypes.data_as(dp), prim.ctypes.data_as(ip)]
    for k in null:
        args[k] = None
    rc = P.lib().ptx_walk_rays(g._h, walk, n, *args)
    if rc != 0:  # nothing was launched, nothing written
        assert (t == -7.0).all() and (prim == -7).all()
    return rc


def test_refusals_leave_the_handle_usable(P, W, oracle):
    from path_tracer_ocaml_amd import abi
    A = abi
    o_scene, g_scene, o, dr = simd_soup(P, oracle, 2, 1.0)
    o, dr = o[:2000], dr[:2000]
    z = np.zeros_like(o)

    def still_exact():
        check_walks(W, o_scene, g_scene, [A.PTX_WALK_SHARED_ASM, A.PTX_WALK_OCT_ASM_TAIL], o, dr)
        check_walks(W, o_scene, g_scene, [A.PTX_WALK_PACKET], z, dr)
    for w in W.ARRAY + [A.PTX_WALK_SHARED_DIV_ZERO]:  # the Array_leaf walk on a Simd_leaf scene
        assert raw_call(P, g_scene, w, z, dr) == ERR_STATE
        assert "Array_leaf" in P.last_error()
    still_exact()
    for w in W.SIMD_ZERO:  # an origin that is not +0.0: -0.0, a tiny number, in the last ray's last component
        for bad in (-0.0, 1e-300, 5e-324):
            zb = z.copy()
            zb[-1, 2] = bad
            assert raw_call(P, g_scene, w, zb, dr) == ERR_ARG
            assert "+0" in P.last_error()
        with pytest.raises(P.PtxError):
            g_scene.walk_rays(w, o, dr)
    still_exact()
    for k in range(4):
        assert raw_call(P, g_scene, A.PTX_WALK_SHARED_ASM, o, dr, null=(k,)) == ERR_ARG
    assert P.lib().ptx_walk_rays(None, 0, 0, None, None, None, None) == ERR_ARG
    for w in (-1, 10, 1 << 20):
        assert raw_call(P, g_scene, w, o, dr) == ERR_ARG
    assert raw_call(P, g_scene, A.PTX_WALK_SHARED_ASM, o, dr, n=-1) == ERR_ARG
    assert raw_call(P, g_scene, A.PTX_WALK_SHARED_ASM, o, dr, n=0) == 0
    still_exact()
    g_scene.close()
    # a Simd_leaf walk on an Array_leaf scene
    rng = np.random.default_rng(21)
    d, keep = make_desc(abi, spheres=sphere_soup(rng, 60, 1.0, np.array([0.0, 0.0, -4.0]), 4.0), leaf_kind=1, cutoff=3)
    o_scene, g_scene = both(P, oracle, d, keep)
    for w in W.SIMD + [A.PTX_WALK_SHARED_ASM_ZERO, A.PTX_WALK_OCT_ASM_ZERO]:
        assert raw_call(P, g_scene, w, z, dr) == ERR_STATE
    check_walks(W, o_scene, g_scene, W.ARRAY, o, dr)
    g_scene.close()
    # a host-only scene
    host = P.Scene(d, -1, keepalive=keep)
    assert raw_call(P, host, A.PTX_WALK_SHARED_DIV, o, dr) == ERR_STATE
    host.close()


def test_a_scene_walked_from_hbm_takes_none_of_the_walks(P, W, oracle):
    from path_tracer_ocaml_amd import abi
    ptr, keep = X.scene_desc("ganesha_150k", oracle, abi)
    g = P.Scene(ptr, 0, keepalive=keep)
    try:
        assert not g.stats()["traversal_in_lds"]
        o, d = np.zeros((64, 3)), np.tile([0.0, 0.0, -1.0], (64, 1))
        for w in sorted(W.names):
            assert raw_call(P, g, w, o, d) == ERR_STATE, W.names[w]
            assert "HBM" in P.last_error()
        t, prim, _ = g.intersect_rays(o, d)  # the handle still works
        t_c, p_c, _ = oracle.Scene(ptr, keep).intersect_rays(o, d)
        assert np.array_equal(prim, p_c) and np.array_equal(bits(t), bits(t_c))
    finally:
        g.close()


def test_the_per_octant_walk_at_its_capacity_bound(P, W, oracle, monkeypatch):
    """test_soups_at_the_capacity_bound's family (tests/test_gpu_lds_oct.py): the last soup whose launch fits with the per-octant
    image walks it, exactly; the first that does not is refused that walk and keeps the others."""
    from path_tracer_ocaml_amd import abi
    monkeypatch.setenv("PTX_LDS_OCT", "1")
    under = over = None
    for n in range(420, 900, 6):
        d, keep = soup_desc(n)
        host = P.Scene(d, -1, keepalive=keep)  # (host-only: the tree's size without a device)
        st = host.stats()
        host.close()
        n64 = keeps_nodes64(st["tree_nodes"], st["leaf_slots"], st["tree_depth"])
        assert n64 is not None
        if not oct_fits(st["tree_nodes"], st["leaf_slots"], n64):
            over = n
            break
        under = n
    assert under is not None and over is not None, "the family did not cross the bound"
    rng = np.random.default_rng(8)
    for n, fits in ((under, True), (over, False)):
        o_scene, g_scene = both(P, oracle, *soup_desc(n))
        assert g_scene.stats()["traversal_in_lds"] == 1
        o, dr = ray_mix(rng, 8000, 1.0, np.array([0.2, -0.1, -5.0]), leaf_boxes(g_scene))
        z = np.zeros_like(o)
        if fits:
            check_walks(W, o_scene, g_scene, W.SIMD, o, dr)
            check_walks(W, o_scene, g_scene, W.SIMD_ZERO, z, dr)
        else:
            for w in W.OCT:
                assert raw_call(P, g_scene, w, z, dr) == ERR_STATE, W.names[w]
                assert "per-octant" in P.last_error()
            check_walks(W, o_scene, g_scene, [w for w in W.SIMD if w not in W.OCT], o, dr)
            check_walks(W, o_scene, g_scene, [w for w in W.SIMD_ZERO if w not in W.OCT], z, dr)
        g_scene.close()


# ---- 9. both tree builders
@pytest.mark.parametrize("builder", [1, 2])
def test_host_built_and_gpu_built_trees(P, W, oracle, builder):
    """the first soup of test_sphere_soups_through_both_assembly_loops with the builder forced (SceneDesc.reserved: 1 host, 2 GPU)"""
    from path_tracer_ocaml_amd import abi
    seed, scale = SOUPS[0]
    rng = np.random.default_rng(1000 + seed)
    centre = rng.uniform(-1.0, 1.0, 3) * scale * 3.0
    sph = sphere_soup(rng, 300, scale, centre)
    d, keep = make_desc(abi, spheres=sph, leaf_kind=0, cutoff=16)
    d.reserved = builder
    o_scene, g_scene = both(P, oracle, d, keep)
    assert bool(g_scene.stats()["bvh_built_on_gpu"]) == (builder == 2)
    boxes = leaf_boxes(g_scene)
    o, dr = ray_mix(rng, 30000, scale, centre, boxes)
    prims = check_walks(W, o_scene, g_scene, W.SIMD, o, dr)
    assert (prims >= 0).sum() > 300 and (prims < 0).sum() > 300
    dz = dirs_from_origin(rng, 10000, scale, centre, boxes, dr, sph)
    prims = check_walks(W, o_scene, g_scene, W.SIMD_ZERO, np.zeros_like(dz), dz)
    assert (prims >= 0).sum() > 500
    g_scene.close()
