"""The camera tile lists (csrc/scene_host.cpp: scene_tile_lists) and the scan of them (csrc/pt_tile_scan.h), without a GPU:
build/asan/tile_lists_driver assembles scenes and builds grids with the code the library ships and runs the scan the kernel runs,
compiled for the host, under AddressSanitizer + UndefinedBehaviorSanitizer.

* The grid against a brute-force restatement: every record's set is the numpy plane test's, its order the order in which a
  near-child-first descent of the tile's octant (test_scene_host's descent, the one check_walk follows) meets the slots' leaves, and
  the walk tiles are exactly the tiles whose direction bounds straddle or touch zero, the tiles with more than 15 candidates and the
  tiles with a candidate whose |c| exceeds 2^18 r.
* The scan against the oracle: (slot, t) of every camera ray the scan answered without a guard equals Scene.intersect_rays' bit for
  bit, over random camera samples and over rays aimed within +-4 ulps at silhouettes, contact points, box corners and faces,
  coincident and tangent spheres, from inside a sphere and with a sphere behind the camera.
* Mutants of the builder (no inflation, lists in slot order; compiled into the driver's build only) fail the first check.  They cannot
  fail the second: a ray that only the inflation keeps right grazes its sphere, and a ray whose hit depends on the list's order ties
  with another hit, so the scan's own guards send both back to the walk.  The restatement carries its own copy of
  the inflation, 2^-40: the constant is justified by its bound, the test pins that builder and statement agree on it.
* Each guard alone is shown to fire (isolated silhouettes: the discriminant's; coincident spheres: the tie's); the scan without its
  guards is run against the adversarial sets and its mismatches are reported (see test_scan_without_guards).
"""
import os

import numpy as np
import pytest

from test_gpu_edge_cases import make_desc
from test_sanitizers import ENV, ROOT, built, run_clean  # noqa: F401  (built: the `make asan` fixture)
from test_scene_host import NODE, descent

REC = np.dtype([("count", "u1"), ("octant", "u1"), ("slot", "<u2", 15)])
HIT = np.dtype([("t", "<f8"), ("slot", "<i4"), ("status", "<i4")])
WALK, MAX_SLOTS, INFLATE, MAX_CR = 0xFF, 15, 2.0 ** -40, 2.0 ** 18
CAMERA = (-1.0, -0.5, 2.0, 1.0)  # make_desc's and the driver's for file: scenes


def scene_arg(tmp_path, scene):
    """'shirley', or an array of (x, y, z, r) rows written for the driver's file: scenes"""
    if isinstance(scene, str):
        return scene
    path = os.path.join(tmp_path, "spheres.bin")
    np.ascontiguousarray(scene, dtype=np.float64).tofile(path)
    return "file:" + path


def grid(built, tmp_path, scene, w, h, *opts):
    out = run_clean([os.path.join(built, "tile_lists_driver"), "grid", scene_arg(tmp_path, scene), str(w), str(h), str(tmp_path), *opts])
    first, second = out.splitlines()
    f = first.split()
    info = {f[i]: int(f[i + 1]) for i in range(0, len(f), 2)}
    info["camera"] = [float.fromhex(x) for x in second.split()[1:]]
    load = lambda name, dt: np.fromfile(os.path.join(tmp_path, name + ".bin"), dtype=dt)  # noqa: E731
    return info, load("nodes", NODE), load("sph", "<f8").reshape(-1, 4), load("slot_prim", "<i4"), load("grid", REC)


def axis_pass(sph, real, n_tiles, extent, ll, v, flip, comp, inflate=INFLATE):
    """One side of the grid: per tile column (row) the bounds of ll + v c over its pixels and the slots that pass both planes"""
    t = np.arange(n_tiles, dtype=np.float64)
    scale = 1.0 / float(extent)
    p0, p1 = (8.0 * t) * scale, np.minimum(8.0 * t + 8.0, float(extent)) * scale
    a = ll + v * ((1.0 - p0) if flip else p0)
    b = ll + v * ((1.0 - p1) if flip else p1)
    lo, hi = np.minimum(a, b), np.maximum(a, b)
    nlo, nhi = np.sqrt(1.0 + lo * lo), np.sqrt(1.0 + hi * hi)
    r = np.abs(sph[:, 3])
    length = np.sqrt(((sph[:, 0] * sph[:, 0]) + (sph[:, 1] * sph[:, 1])) + (sph[:, 2] * sph[:, 2]))
    e = r + inflate * (length + r) if inflate else r
    dl = sph[None, :, comp] + lo[:, None] * sph[None, :, 2]
    dh = sph[None, :, comp] + hi[:, None] * sph[None, :, 2]
    with np.errstate(invalid="ignore"):
        out = (dl < -(e[None, :] * nlo[:, None])) | (dh > e[None, :] * nhi[:, None])
    return lo, hi, ~out & real[None, :]


def slot_ranks(nodes, n_slots):
    """rank[o][slot]: the slot's position in the order octant o's near-first descent meets the leaves (slot order inside a leaf)"""
    ranks = np.zeros((4, n_slots), dtype=np.int64)
    for o in range(4):
        order, _ = descent(nodes, o)
        k = 0
        for node in order:
            if int(nodes["b"][node]) >> 30 == 3:
                first, count = int(nodes["a"][node]), int(nodes["b"][node]) & 0x3FFFFFFF
                ranks[o, first:first + count] = np.arange(k, k + count)
                k += count
        assert k == n_slots
    return ranks


def check_grid(built, tmp_path, scene, w, h, *opts):
    """The records of the driver's grid against the restatement; returns (info, per-tile list lengths with -1 for walk tiles, per-tile
    candidate counts of the restatement, strict sign-change tiles)"""
    info, nodes, sph, slot_prim, rec = grid(built, tmp_path, scene, w, h, *opts)
    tx, ty = (w + 7) // 8, (h + 7) // 8
    assert (info["tiles_x"], info["tiles_y"], len(rec)) == (tx, ty, tx * ty)
    llx, lly, vx, vy = info["camera"]
    real = slot_prim >= 0
    assert np.array_equal(real, ~np.isnan(sph[:, 3]))  # NaN padding is exactly the slots without a primitive
    xlo, xhi, cols = axis_pass(sph, real, tx, w, llx, vx, False, 0)
    ylo, yhi, rows = axis_pass(sph, real, ty, h, lly, vy, True, 1)
    ranks = slot_ranks(nodes, len(sph))
    with np.errstate(invalid="ignore"):
        length = np.sqrt(((sph[:, 0] * sph[:, 0]) + (sph[:, 1] * sph[:, 1])) + (sph[:, 2] * sph[:, 2]))
        odd = real & ~(np.isfinite(length) & np.isfinite(sph[:, 3]) & (length <= MAX_CR * np.abs(sph[:, 3])))
    mixed_x, mixed_y = (xlo <= 0.0) & (xhi >= 0.0), (ylo <= 0.0) & (yhi >= 0.0)
    strict = ((xlo < 0.0) & (xhi > 0.0))[None, :] | ((ylo < 0.0) & (yhi > 0.0))[:, None]
    counts, cands = np.zeros((ty, tx), dtype=np.int64), np.zeros((ty, tx), dtype=np.int64)
    for j in range(ty):
        for i in range(tx):
            r = rec[j * tx + i]
            want = np.flatnonzero(cols[i] & rows[j])
            cands[j, i] = len(want)
            walk = bool(mixed_x[i] or mixed_y[j] or len(want) > MAX_SLOTS or odd[want].any())
            assert (r["count"] == WALK) == walk, (i, j, r["count"], len(want))
            if walk:
                counts[j, i] = -1
                continue
            o = (1 if xlo[i] > 0.0 else 0) | (2 if ylo[j] > 0.0 else 0)
            assert r["octant"] == o and r["count"] == len(want), (i, j)
            want = want[np.argsort(ranks[o, want], kind="stable")]
            assert np.array_equal(r["slot"][:len(want)], want), (i, j, o)
            assert not r["slot"][len(want):].any()
            counts[j, i] = len(want)
    assert info["walk"] == int((counts < 0).sum()) and info["longest"] == max(0, int(counts.max()))
    return info, counts, cands, strict


def soup(n, seed=11):
    from test_gpu_fuzz import sphere_soup
    rng = np.random.default_rng(seed)  # (off the image's centre, whose tile row and columns keep the walk: their bounds straddle or touch zero)
    return np.array([s[:4] for s in sphere_soup(rng, n, 1.0, np.array([1.8, 1.0, -5.0]), 1.0)])


@pytest.mark.parametrize("w,h", [(1920, 1080), (600, 300), (61, 37)])
def test_shirley_grid_equals_the_restatement(built, tmp_path, w, h):
    info, counts, cands, strict = check_grid(built, tmp_path, "shirley", w, h)
    assert (info["nodes"], info["slots"]) == (341, 684)
    if (w, h) == (1920, 1080):
        # the figures the change was sized with: 1.91 spheres per tile, median 2, 99th percentile 6, at most 9, 14 % of the tiles
        # empty, 240 tiles with a sign change inside (the tile row across the horizon); the two tile columns whose common bound
        # is exactly zero keep the walk too
        # (candidate sets of all 32 400 tiles, the walk tiles' included)
        print("tiles", cands.size, "walk", info["walk"], "mean", cands.mean(), "mean of the lists", counts[counts >= 0].mean(), "median", np.median(cands),
              "p99", np.percentile(cands, 99), "max", cands.max(), "empty", (cands == 0).mean())
        assert int(strict.sum()) == 240 and info["walk"] == 240 + 2 * 135 - 2
        assert round(float(cands.mean()), 3) == 1.910
        assert np.median(cands) == 2 and np.percentile(cands, 99) == 6 and cands.max() == 9
        assert round(float((cands == 0).mean()), 2) == 0.14


@pytest.mark.parametrize("n", [1, 2, 17, 300])
def test_soup_grid_equals_the_restatement(built, tmp_path, n):
    info, counts, cands, _ = check_grid(built, tmp_path, soup(n), 64, 40)
    assert info["slots"] >= n and (cands > 0).any()
    if n == 17:
        assert (counts > 0).any()  # lists that hold something
    if n == 300:
        assert (cands > MAX_SLOTS).any()  # a dense soup: tiles that overflow a record and keep the walk


def stacked(n=40):
    """n small spheres in a row behind the centre of one tile of a 64 x 40 image: more candidates than a record holds"""
    z = -3.0 - 0.25 * np.arange(n)
    x, y = 0.45 * -z, 0.31 * -z  # on one camera ray: X = 0.45, Y = 0.31, pixel (46.4, 7.6): tile (5, 0)
    return np.stack([x, y, z, np.full(n, 0.05)], axis=1)


def test_overflow_tiles_walk(built, tmp_path):
    info, counts, _, strict = check_grid(built, tmp_path, stacked(), 64, 40)
    assert counts[0, 5] == -1 and not strict[0, 5] and info["longest"] <= MAX_SLOTS


def test_a_sphere_far_smaller_than_its_distance_walks(built, tmp_path):
    """|c| = 5.4 > 2^18 r: the guard on the discriminant is not sized for it, so the tiles that would list it keep the walk; its
    neighbour's other tiles keep their lists"""
    spheres = np.array([[1.8, 1.0, -5.0, 1e-5], [2.2, 1.4, -5.0, 0.3]])
    info, counts, cands, strict = check_grid(built, tmp_path, spheres, 64, 40)
    # pixel (43.5, 12.0): tile (5, 1)
    assert counts[1, 5] == -1 and not strict[1, 5] and 0 < cands[1, 5] <= MAX_SLOTS
    assert (counts > 0).any()


def tangent_soup():
    """One sphere just outside the left plane of tile column 5 of a 64-pixel-wide image (X = -1 + 2 * 40 / 64 = 0.25), nearer to it than
    the inflation (2^-40 (|c| + r)) but farther than rounding, and one sphere well inside the image so that the tree has two leaves' worth"""
    X, r, z = 0.25, 0.125, -4.0
    n = np.sqrt(1.0 + X * X)
    x = X * -z - (r * (1.0 + 2.0 ** -44)) * n  # c.x + X c.z = -(r + r 2^-44) sqrt(1 + X^2)
    return np.array([[x, 0.8, z, r], [0.6, -0.2, -5.0, 0.3]])  # (y: tile row 1, clear of the row across the horizon)


def test_mutants_of_the_builder_fail(built, tmp_path):
    """no inflation: the tangent sphere drops out of the tiles the restatement lists it in; slot order: Shirley's lists come out in
    another order than the descent's.  Both pass unmutated."""
    check_grid(built, tmp_path, tangent_soup(), 64, 40)
    with pytest.raises(AssertionError):
        check_grid(built, tmp_path, tangent_soup(), 64, 40, "mutant=1")
    check_grid(built, tmp_path, "shirley", 61, 37)
    with pytest.raises(AssertionError):
        check_grid(built, tmp_path, "shirley", 61, 37, "mutant=2")


# ---------------------------------------------------------------- the scan against the oracle
def ulp_steps(x, k):
    x = np.array(x, dtype=np.float64)
    for _ in range(abs(k)):
        x = np.nextafter(x, np.inf if k > 0 else -np.inf)
    return x


def aim(points, camera, w, h):
    """Pixel coordinates of the camera samples whose rays pass through `points`, each moved by -4 .. 4 ulps in both coordinates; the
    ones outside the image are dropped"""
    llx, lly, vx, vy = camera
    p = np.asarray(points, dtype=np.float64).reshape(-1, 3)
    p = p[p[:, 2] < 0.0]
    px = ((p[:, 0] / -p[:, 2]) - llx) / vx * w
    py = (1.0 - ((p[:, 1] / -p[:, 2]) - lly) / vy) * h
    out = [np.stack([ulp_steps(px, k), ulp_steps(py, j)], axis=1) for k in range(-4, 5) for j in (-4, 0, 4)]
    s = np.concatenate(out)
    return s[(s[:, 0] >= 0.0) & (s[:, 0] < w) & (s[:, 1] >= 0.0) & (s[:, 1] < h)]


def silhouettes(spheres, n_angles=12):
    """Points where rays from the origin touch each sphere"""
    out = []
    for x, y, z, r in spheres:
        c = np.array([x, y, z])
        L = np.linalg.norm(c)
        if not L > abs(r):
            continue
        u = c / L
        e1 = np.cross(u, [0.0, 1.0, 0.0] if abs(u[1]) < 0.9 else [1.0, 0.0, 0.0])
        e1 /= np.linalg.norm(e1)
        e2 = np.cross(u, e1)
        s2 = 1.0 - (r / L) ** 2
        for a in np.linspace(0.0, 2.0 * np.pi, n_angles, endpoint=False):
            out.append(c * s2 + abs(r) * np.sqrt(s2) * (np.cos(a) * e1 + np.sin(a) * e2))
    return np.array(out).reshape(-1, 3)


def scan(built, tmp_path, scene, w, h, samples, *opts):
    np.ascontiguousarray(samples, dtype=np.float64).tofile(os.path.join(tmp_path, "samples.bin"))
    run_clean([os.path.join(built, "tile_lists_driver"), "scan", scene_arg(tmp_path, scene), str(w), str(h), str(tmp_path), *opts], timeout=900)
    dirs = np.fromfile(os.path.join(tmp_path, "dirs.bin"), dtype="<f8").reshape(-1, 3)
    return dirs, np.fromfile(os.path.join(tmp_path, "hits.bin"), dtype=HIT)


def compare(o_scene, slot_prim, dirs, hits):
    """-> (rays the scan answered, how many of them differ from the oracle in slot or in the bits of t, rays a guard sent back)"""
    t, prim, _ = o_scene.intersect_rays(np.zeros_like(dirs), dirs)
    done = hits["status"] == 0
    mine = np.where(hits["slot"] >= 0, slot_prim[np.maximum(hits["slot"], 0)], -1)
    bad = done & ((mine != prim) | (hits["t"].view(np.uint64) != t.view(np.uint64)))
    return int(done.sum()), int(bad.sum()), int((hits["status"] == 1).sum())


@pytest.fixture(scope="module")
def shirley_sets(built, oracle, tmp_path_factory):
    """The Shirley ray sets at 1920 x 1080, made once: name -> samples"""
    tmp = tmp_path_factory.mktemp("shirley_sets")
    info, nodes, sph, slot_prim, _ = grid(built, tmp, "shirley", 1920, 1080)
    cam, w, h = info["camera"], 1920, 1080
    real = sph[slot_prim >= 0]
    rng = np.random.default_rng(2024)
    ground = real[np.argmax(real[:, 3])]
    small = real[real[:, 3] < 10.0]
    toward = small[:, :3] - ground[None, :3]
    contact = ground[None, :3] + toward / np.linalg.norm(toward, axis=1, keepdims=True) * ground[3]
    mn, mx = nodes["mn"], nodes["mx"]
    corners = np.array([[(mn, mx)[i][k, 0], (mn, mx)[j][k, 1], (mn, mx)[l][k, 2]] for k in range(len(nodes)) for i in (0, 1) for j in (0, 1) for l in (0, 1)])
    mid = 0.5 * (mn + mx)
    faces = np.array([np.where(np.arange(3) == a, (mn, mx)[s][k], mid[k]) for k in range(len(nodes)) for a in range(3) for s in (0, 1)])
    sets = {
        "random": np.stack([rng.uniform(0.0, w, 4_000_000), rng.uniform(0.0, h, 4_000_000)], axis=1),
        "silhouettes": aim(silhouettes(real), cam, w, h),
        "contacts": aim(contact, cam, w, h),
        "corners": aim(corners, cam, w, h),
        "faces": aim(faces, cam, w, h),
    }
    sets["random"] = sets["random"][(sets["random"][:, 0] < w) & (sets["random"][:, 1] < h)]
    return sets, slot_prim


def run_sets(built, oracle, tmp_path, scene, o_scene, slot_prim, w, h, sets, *opts):
    names = list(sets)
    dirs, hits = scan(built, tmp_path, scene, w, h, np.concatenate([sets[k] for k in names]), *opts)
    out, at = {}, 0
    for k in names:
        n = len(sets[k])
        out[k] = compare(o_scene, slot_prim, dirs[at:at + n], hits[at:at + n]) + (n,)
        at += n
    return out


def test_scan_equals_the_oracle_on_shirley(built, oracle, tmp_path, shirley_sets):
    sets, slot_prim = shirley_sets
    d = oracle.desc_shirley(1920, 1080)
    res = run_sets(built, oracle, tmp_path, "shirley", oracle.Scene(d.ptr, d), slot_prim, 1920, 1080, sets)
    for k, (done, bad, guards, n) in res.items():
        print(k, "rays", n, "scanned", done, "mismatches", bad, "guards", guards)
    assert sum(r[3] for r in res.values()) >= 4_000_000
    for k, (done, bad, guards, n) in res.items():
        assert bad == 0 and done > 0, k
    assert res["silhouettes"][2] > 0  # grazing rays: the guards send them back
    assert res["random"][2] < 1e-4 * res["random"][3]
    assert res["random"][0] > 0.95 * res["random"][3]  # the lists answer nearly every camera ray


def special_soups():
    """name -> (spheres, points to aim at).  make_desc's camera looks down -z with X in [-1, 1], Y in [-0.5, 0.5]"""
    # (everything off the image's centre: the tile row and the two tile columns there keep the walk)
    two = np.array([[2.0, 1.2, -4.0, 0.5], [2.0, 1.2, -4.0, 0.5], [1.6, 0.9, -5.0, 0.4], [2.4, 0.9, -5.0, 0.4], [3.5, 2.1, -7.0, 0.2]])
    inside = np.array([[0.0, 0.0, -0.5, 2.0], [0.6, 0.35, -1.2, 0.3], [-0.8, -0.5, -1.6, 0.2]])
    behind = np.array([[1.5, 0.9, 3.0, 1.0], [1.8, 1.2, -4.0, 0.5], [-3.0, -1.5, -6.0, 0.6]])
    touch = np.array([[2.0, 0.9, -5.0]])  # where the two tangent spheres meet
    return {
        "coincident_tangent": (two, np.concatenate([silhouettes(two), two[:, :3], touch])),
        "inside": (inside, np.concatenate([silhouettes(inside[1:]), inside[1:, :3]])),
        "behind": (behind, np.concatenate([silhouettes(behind[1:]), behind[1:, :3], -behind[:1, :3]])),
    }


def soup_sets(built, tmp_path, spheres, points, w, h):
    info, _, _, slot_prim, _ = grid(built, tmp_path, spheres, w, h)
    rng = np.random.default_rng(5)
    sets = {"aimed": aim(points, info["camera"], w, h), "random": np.stack([rng.uniform(0.0, w, 20000), rng.uniform(0.0, h, 20000)], axis=1)}
    return sets, slot_prim


@pytest.mark.parametrize("name", ["coincident_tangent", "inside", "behind"])
def test_scan_equals_the_oracle_on_special_soups(built, oracle, tmp_path, name):
    import ctypes as C
    from path_tracer_ocaml_amd import abi
    spheres, points = special_soups()[name]
    w, h = 64, 40
    sets, slot_prim = soup_sets(built, tmp_path, spheres, points, w, h)
    d, keep = make_desc(abi, spheres=[(*s, 0) for s in spheres], leaf_kind=0, cutoff=16)
    res = run_sets(built, oracle, tmp_path, spheres, oracle.Scene(C.pointer(d), keep), slot_prim, w, h, sets)
    for k, (done, bad, guards, n) in res.items():
        print(name, k, "rays", n, "scanned", done, "mismatches", bad, "guards", guards)
        assert bad == 0 and n > 0, (name, k)
    if name == "coincident_tangent":
        assert res["random"][2] > 0  # rays through the middle of the coincident pair tie with the closest hit so far: the tie guard alone
    if name == "behind":
        assert res["aimed"][2] > 0  # silhouettes of spheres with nothing in front or behind: the discriminant's guard alone


def test_scan_without_guards(built, oracle, tmp_path, shirley_sets):
    """The mutant with the guards off, against the silhouette, coincident and tangent sets.  MEASURED (printed below): it differs from
    the oracle on none of these rays -- the list order reproduces the walk's ties, and a box test that fails by an ulp next to a
    grazing hit did not occur among them.  The guards stay: they cover what rounding can do, not what these sets happened to do.
    The test pins that guards=0 switches them off on exactly these sets; that the guarded scan sends rays of the same sets back
    is asserted where those sets are scanned with the guards (the two tests above)."""
    import ctypes as C
    from path_tracer_ocaml_amd import abi
    sets, slot_prim = shirley_sets
    adversarial = {k: v for k, v in sets.items() if k != "random"}
    d = oracle.desc_shirley(1920, 1080)
    res = run_sets(built, oracle, tmp_path, "shirley", oracle.Scene(d.ptr, d), slot_prim, 1920, 1080, adversarial, "guards=0")
    total_bad = sum(r[1] for r in res.values())
    spheres, points = special_soups()["coincident_tangent"]
    s2, sp2 = soup_sets(built, tmp_path, spheres, points, 64, 40)
    dd, keep = make_desc(abi, spheres=[(*s, 0) for s in spheres], leaf_kind=0, cutoff=16)
    res2 = run_sets(built, oracle, tmp_path, spheres, oracle.Scene(C.pointer(dd), keep), sp2, 64, 40, s2, "guards=0")
    total_bad += sum(r[1] for r in res2.values())
    print("guards off: mismatches", total_bad, {k: r[:3] for k, r in {**res, **res2}.items()})
    assert all(r[2] == 0 for r in {**res, **res2}.values())  # guards=0 really switches them off
