"""The oracle's photon mapper (oracle/pt_oracle.c, orc_ppm_render) against things that do not share its code: a brute-force
gather in extended precision over its own photon list and eye hits (tests/ppm_reference.py), the radius schedule in exact
rationals, and the rays the lights send out.  CPU only.  The GPU is pinned to the oracle bit for bit in test_gpu_ppm.py, so a
mistake the two restatements share -- pruning in the tree walk, the wrong iteration's radius, a dropped normal test, the cone
weight, the normaliser, the flip -- has to get past this file."""
import math
from fractions import Fraction

import numpy as np
import pytest

import ppm_reference as R
from path_tracer_ocaml_amd import abi

run_case = R.run_case


@pytest.mark.parametrize("name", R.CASES)
def test_dump_is_the_same_run(oracle, name):
    """The exports are taps: the image, the counters and the last radius of a dumping run are orc_ppm_render's own."""
    run = run_case(oracle, name)
    for it, dmp in enumerate(run["dumps"]):
        assert np.array_equal(dmp["img"].view(np.uint64), run["img"].view(np.uint64))
        assert dmp["stats"] == {k: run["stats"][k] for k in dmp["stats"]}
    assert run["dumps"][-1]["radius"] == run["stats"]["last_radius"]
    assert sum(len(dmp["center"]) for dmp in run["dumps"]) == run["stats"]["photons_stored"]
    assert sum(int(dmp["neighbors"].sum()) for dmp in run["dumps"]) == run["stats"]["neighbors"]


@pytest.mark.parametrize("name", R.CASES)
def test_neighbour_counts_enclosed_by_brute_force(oracle, name):
    run = run_case(oracle, name)
    total_in = total_und = 0
    for it, (dmp, g) in enumerate(zip(run["dumps"], run["gathers"])):
        nb = dmp["neighbors"]
        assert (nb[~dmp["diffuse"]] == 0).all()
        low = nb < g["inside"]
        high = nb > g["inside"] + g["undecided"]
        assert not low.any() and not high.any(), (name, it, int(low.sum()), int(high.sum()), np.nonzero(low | high)[0][:5])
        total_in += int(g["inside"].sum())
        total_und += int(g["undecided"].sum())
        print(f"{name} iteration {it}: radius {dmp['radius']:.6g} photons {len(dmp['center'])} inside {int(g['inside'].sum())} "
              f"undecided {int(g['undecided'].sum())} exact-arithmetic pairs {g['n_exact']}")
    assert total_in <= run["stats"]["neighbors"] <= total_in + total_und
    assert total_in > 0


@pytest.mark.parametrize("name", R.CASES)
def test_values_within_the_bound_of_brute_force(oracle, name):
    run = run_case(oracle, name)
    p = run["params"]
    inv = R.LD(1.0 / p.photon_count)  # the oracle multiplies by the binary64 1 / photon_count: one of the bound's roundings
    worst = 0.0
    for it, (dmp, g) in enumerate(zip(run["dumps"], run["gathers"])):
        clean = g["undecided"] == 0
        err = np.abs(dmp["estimate"].astype(R.LD) * inv - g["estimate"])
        bad = (err > g["bound"]) & clean[:, None]
        assert not bad.any(), (name, it, int(bad.sum()))
        lit = (g["bound"] > 0) & clean[:, None]
        worst = max(worst, float((err[lit] / g["bound"][lit]).max()))
        dark = (g["inside"] == 0) & clean
        assert (dmp["estimate"][dark] == 0.0).all()
    ref, bnd, clean, dark = run["frame"]
    img = run["img"]
    lit = ((ref > 0) | (img > 0)).any(axis=2)
    excluded = lit & ~clean
    assert excluded.sum() <= 0.01 * lit.sum(), (int(excluded.sum()), int(lit.sum()))
    err = np.abs(img.astype(R.LD) - ref)
    use = (lit & clean)[:, :, None] & np.ones(3, dtype=bool)
    assert use.any()
    assert (err[use] <= bnd[use]).all(), (name, float((err[use] / np.maximum(bnd[use], R.LD(1e-300))).max()))
    assert (img[dark] == 0.0).all()
    pos = use & (bnd > 0)
    print(f"{name}: lit pixels {int(lit.sum())} excluded {int(excluded.sum())} worst error / bound: per iteration {worst:.3f}, "
          f"frame {float((err[pos] / bnd[pos]).max()):.3f}")


def _within_ulps(x, exact_square, ulps):
    """|x - sqrt(exact_square)| <= ulps * ulp(x), decided in rationals."""
    step = Fraction(math.ulp(x)) * ulps
    lo, hi = Fraction(x) - step, Fraction(x) + step
    return lo > 0 and lo * lo <= exact_square <= hi * hi


@pytest.mark.parametrize("alpha", [2.0 / 3.0, 1.0, 0.0])
def test_radius_schedule_against_exact_rationals(oracle, alpha):
    """radius i = sqrt(prod_{k < i} (k + alpha) / k * init_radius2 / i), i = 1 .. 50, within 4 ulp; alpha = 1 is constant and
    alpha = 0 is r1 / sqrt(i)."""
    w = h = 4
    d = oracle.desc_cornell(w, h, 0.0)
    sc = oracle.Scene(d.ptr, d)
    lights = oracle.lights_cornell(w, h)
    init = Fraction(sc.ppm_dump(abi.ppm_params(w, h, iterations=1, photon_count=64, alpha=alpha), lights, 0)["init_radius2"])
    a = Fraction(alpha)
    product = Fraction(1)
    for i in range(1, 51):
        if i > 1:
            product = product * (Fraction(i - 1) + a) / (i - 1)
        _, st = sc.ppm_render(abi.ppm_params(w, h, iterations=i, photon_count=64, alpha=alpha), lights)
        r = st["last_radius"]
        assert _within_ulps(r, product * init / i, 4), (alpha, i, r)
        if alpha == 1.0:
            assert _within_ulps(r, init, 4), (i, r)
        if alpha == 0.0:
            assert _within_ulps(r, init / i, 4), (i, r)


@pytest.mark.parametrize("name", ["cornell", "ganesha", "shirley"])
def test_init_radius2_is_the_mean_extent_over_the_mean_side(oracle, name):
    """init_radius2 = (mean bbox extent / ((W + H) / 2))^2.  The binary64 evaluation rounds the three extents, two additions,
    two divisions and the square: at most 2 (1 + 2 + 1 + 1) + 1 = 11 half-ulps relative, which 8 ulp covers."""
    run = run_case(oracle, name)
    p, bb = run["params"], [Fraction(float(v)) for v in run["bbox"]]
    exact = ((bb[3] - bb[0] + bb[4] - bb[1] + bb[5] - bb[2]) / 3 / Fraction(p.width + p.height, 2)) ** 2
    got = run["dumps"][0]["init_radius2"]
    assert abs(Fraction(got) - exact) <= 8 * Fraction(math.ulp(got))
    assert run["dumps"][0]["radius"] == math.sqrt(got)


# ---- the photon pass: max_bounces = 1, so every photon is the first hit of its path ----
def _inside_ground(O):
    """The Shirley scene for lights INSIDE its ground sphere (returns the sphere's centre in camera space, where lights live).
    This leans on one property of the restated sphere test, sphere_intersect in oracle/pt_oracle.c: for an origin inside
    (c = |f|^2 - r^2 <= 0) it returns t_hit = q / a with q = bp + sign(bp) sqrt(a discrim), bp = (centre - origin) . direction,
    which is negative, hence no hit, exactly when bp < 0.  So a ray that starts inside is answered only when it heads towards
    the centre's side; its first hit is then the inner side of that diffuse sphere, and with max_bounces = 1 it stores exactly
    one photon.  A ray that heads away sees no ground at all; it could still meet one of the small spheres that sit on the
    ground, which none does from the positions used here (the tests assert the exact set of stored paths, so a change in
    either would show)."""
    w, h = 16, 8
    d = O.desc_shirley(w, h)
    bb = O.Scene(d.ptr, d).tree()[0][0]  # the ground sphere spans the scene's box in x and z
    radius = 0.5 * (bb[3] - bb[0])
    assert radius >= 500 and abs(0.5 * (bb[5] - bb[2]) - radius) < 1e-6 * radius
    centre = np.array([0.5 * (bb[0] + bb[3]), bb[1] + radius, 0.5 * (bb[2] + bb[5])])
    tex_max = d.arrays()["textures"][:, 3:9].reshape(-1, 2, 3).max(axis=(0, 1))
    return d, w, h, centre, tex_max


def _first_hits(O, d, w, h, lights, photon_count):
    p = abi.ppm_params(w, h, iterations=1, photon_count=photon_count, max_bounces=1)
    return O.Scene(d.ptr, d).ppm_dump(p, lights, 0)


def _unit(v):
    return v / np.linalg.norm(v, axis=1)[:, None]


def test_point_light_directions_are_uniform_on_the_sphere(oracle):
    d, w, h, centre, tex_max = _inside_ground(oracle)
    off = np.array([100.0, 200.0, -50.0])
    n = 4000
    dirs, paths = [], []
    for pos in (centre + off, centre - off):  # each sees the hemisphere of directions that faces the centre: together, all
        light = abi.Light()
        light.kind = abi.PTX_LIGHT_POINT
        light.position[:] = list(pos)
        light.color[:] = [1.0, 0.5, 0.25]
        light.power = 8.0
        dmp = _first_hits(oracle, d, w, h, [light], n)
        assert dmp["stats"]["photon_rays"] == n
        assert (np.diff(dmp["path"]) < 0).all()  # the consed list: paths in descending order, one photon each
        # flux: colour x power x the texture's colour, at most its maximum (two roundings)
        cap = np.array([1.0, 0.5, 0.25]) * 8.0 * tex_max
        assert (dmp["flux"] <= cap * (1 + 4 * R.U)).all() and (dmp["flux"] >= 0).all() and dmp["flux"].max() > 0
        dirs.append(_unit(dmp["center"] - pos))
        paths.append(dmp["path"])
    # the two sample coordinates of a path do not depend on the light: every path is answered from exactly one of the two sides
    assert np.array_equal(np.sort(np.concatenate(paths)), np.arange(n))
    assert min(len(q) for q in paths) > n // 3
    dirs = np.concatenate(dirs)
    # a uniform direction has variance 1/3 per component: the standard error of the mean of n of them is sqrt(1 / (3 n))
    assert (np.abs(dirs.mean(axis=0)) <= 4 * math.sqrt(1.0 / (3 * n))).all(), dirs.mean(axis=0)
    # second moments 1/3 (the variance of x^2 is 4/45)
    assert (np.abs((dirs * dirs).mean(axis=0) - 1.0 / 3.0) <= 4 * math.sqrt(4.0 / 45.0 / n)).all()
    # and the closed form of Point_light.random_direction on the path's own two sample coordinates (dimension 2 + 2 * 1)
    q = np.concatenate(paths)
    u, v = oracle.lds_get_vec(4, q, np.zeros_like(q)), oracle.lds_get_vec(4, q, np.ones_like(q))
    theta, phi = 2.0 * np.pi * u, np.arccos(1.0 - 2.0 * v)
    want = np.stack([np.sin(phi) * np.cos(theta), np.sin(phi) * np.sin(theta), np.cos(phi)], axis=1)
    assert np.abs(dirs - want).max() <= 1e-12


@pytest.mark.parametrize("axis", [(0.0, 0.0, 1.0), (0.0, 0.0, -1.0), (0.3, -0.5, 0.2)])
def test_spot_light_stays_inside_its_cone(oracle, axis):
    """Spot_light: directions (x, y, 1) with x^2 + y^2 <= atan(pi / 8)^2 in the light's shader space, i.e. within
    atan(atan(pi / 8)) of the axis.  +z and -z are the two pole branches of Shader_space.create."""
    d, w, h, centre, _ = _inside_ground(oracle)
    ax = np.array(axis) / np.linalg.norm(axis)
    pos = centre - 300.0 * ax  # the whole cone heads towards the centre's side
    light = abi.Light()
    light.kind = abi.PTX_LIGHT_SPOT
    light.position[:] = list(pos)
    light.direction[:] = [3.0 * c for c in axis]  # not normalised: Spot_light.create normalises
    light.color[:] = [1.0, 1.0, 1.0]
    light.power = 5.0
    n = 2000
    dmp = _first_hits(oracle, d, w, h, [light], n)
    assert len(dmp["center"]) == n and dmp["stats"]["photon_rays"] == n
    dirs = _unit(dmp["center"] - pos)
    cos_to_axis = dirs @ ax
    half_angle = math.atan(math.atan(math.pi / 8))
    assert (cos_to_axis >= math.cos(half_angle) - 1e-12).all(), float(cos_to_axis.min())
    # the disk is filled to its rim (u runs over [0, 1)) and all the way round
    assert cos_to_axis.min() <= math.cos(half_angle * 0.98)
    side = dirs - cos_to_axis[:, None] * ax
    assert (np.abs(side.mean(axis=0)) <= 4 * math.sin(half_angle) / math.sqrt(2 * n) + 1e-12).all()


@pytest.mark.parametrize("name", R.CASES)
def test_paths_store_at_most_max_bounces_photons_in_consed_order(oracle, name):
    run = run_case(oracle, name)
    p = run["params"]
    colour = np.zeros(3)
    for l in run["lights"]:
        colour = np.maximum(colour, np.array(l.color[:]) * l.power)
    for it, dmp in enumerate(run["dumps"]):
        path = dmp["path"]
        assert (np.diff(path) <= 0).all()
        assert path.min() >= it * p.photon_count and path.max() < (it + 1) * p.photon_count
        assert np.bincount(path - it * p.photon_count).max() <= p.max_bounces
        # no texture of these scenes exceeds 1, every later factor (specular attenuation, colour / max colour) is <= 1
        assert (dmp["flux"] >= 0).all() and (dmp["flux"] <= colour * (1 + 64 * R.U)).all()


def test_photons_per_light_truncate(oracle):
    """Three equal lights and photon_count = 1000: Int.of_float (1000 * (1/3)) = 333 each, 999 paths in all."""
    d, w, h, centre, _ = _inside_ground(oracle)
    lights = []
    for k in range(3):
        light = abi.Light()
        light.kind = abi.PTX_LIGHT_POINT
        light.position[:] = list(centre + np.array([100.0 + 40.0 * k, 200.0, -50.0]))
        light.color[:] = [1.0, 1.0, 1.0]
        light.power = 2.0
        lights.append(light)
    dmp = _first_hits(oracle, d, w, h, lights, 1000)
    assert dmp["stats"]["photon_rays"] == 999
    path = dmp["path"]
    assert (np.diff(path) < 0).all() and path.min() >= 0 and path.max() <= 998
    # path i belongs to light i // 333, and its photon lies on the ray that light's table entry gives it: the same two sample
    # coordinates from another position give another first hit
    solo = [_first_hits(oracle, d, w, h, [l], 1000) for l in lights]
    for k in range(3):
        sel = (path >= 333 * k) & (path < 333 * (k + 1))
        assert sel.sum() > 50
        own = solo[k]
        at = {int(q): j for j, q in enumerate(own["path"])}
        rows = [at[int(q)] for q in path[sel]]
        assert np.array_equal(own["center"][rows], dmp["center"][sel])
