"""Sphere light sampling (include/ptx.h, "cone-sampling emissive spheres in PTX_LIGHTING_SAMPLED") without a GPU:

* the numpy restatement (tests/spherelight_reference.py) and the C one (tests/c/spherelight_oracle.c) agree bit for bit on the joined
  table and on sample / pd over 2^16 inputs, and the library's own table (host-only scenes) equals both;
* the light triangles keep the bits they have without the option;
* the pd is a density, and every sampled direction has a positive one;
* a Lambertian plane under unoccluded sphere lamps converges to the closed form, and two wrong rules do not;
* modes 1 and 2 estimate the same frame mean, and sampling lowers the variance on a small lamp;
* what the setter refuses, and that a refusal changes nothing.
"""
import ctypes as C
import os

import numpy as np
import pytest

import envlight_support as ES
import lighting_support as LS
import spherelight_reference as R
import spherelight_support as S

bits = S.bits
ROOT = S.ROOT
OLD_MESSAGE = "sampled lighting needs an emissive triangle in the tree (emissive spheres and floor triangles are not sampled)"


@pytest.fixture(scope="module")
def P():
    import path_tracer_ocaml_amd as P
    return P


def _mixed(oracle, n_spheres=3, seed=3):
    """cornell (two ceiling triangles) with n emissive spheres inside the box"""
    rng = np.random.default_rng(seed)
    sp = [(rng.uniform(-0.3, 0.3), rng.uniform(-0.3, 0.3), rng.uniform(-1.8, -1.2), rng.uniform(0.02, 0.1), 10.0, 1.0) for _ in range(n_spheres)]
    d, keep = S.with_spheres(oracle.desc_cornell(32, 16), sp)
    return C.pointer(d), (d, keep)


def _spheres_only(oracle, n, seed=4):
    rng = np.random.default_rng(seed)
    sp = [(rng.uniform(-6, 6), rng.uniform(-6, 6), rng.uniform(-12, -4), rng.uniform(0.05, 0.6), 5.0, 1.0) for _ in range(n)]
    d, keep = S.with_spheres(oracle.desc_shirley(32, 16, no_simd=True), sp)
    return C.pointer(d), (d, keep)


LISTS = {"mixed": lambda o: _mixed(o), "one sphere": lambda o: _spheres_only(o, 1), "64 spheres": lambda o: _spheres_only(o, 64)}


def _numpy_table(rest):
    _, _, tri, sph, _ = rest.table()
    return R.table(tri[:, :9], sph[:, :4])


def _points_and_dirs(tab, n, seed):
    """points around and inside the lights, the sampler pairs, and directions: uniform ones and ones towards the lights"""
    rng = np.random.default_rng(seed)
    centres = np.concatenate([tab.sph[:, :3], tab.tri[:, :3]]) if len(tab.tri) else tab.sph[:, :3]
    radii = np.concatenate([tab.sph[:, 3], np.full(len(tab.tri), 0.3)]) if len(tab.tri) else tab.sph[:, 3]
    pick = rng.integers(0, len(centres), n)
    scale = np.where(rng.uniform(size=n) < 0.2, rng.uniform(0.0, 1.0, n), rng.uniform(1.0, 30.0, n))  # a fifth inside the light
    p = centres[pick] + ES.uniform_directions(n, seed + 1) * (radii[pick] * scale)[:, None]
    uv = np.stack([rng.uniform(0.0, 0.5, n), rng.uniform(0.0, 1.0, n)], axis=1)
    uv[:16] = [(a, b) for a in (0.0, 0.25, 0.5 - 2.0 ** -54, 0.125) for b in (0.0, 0.5, 1.0 - 2.0 ** -53, 0.25)]
    return p, uv, ES.uniform_directions(n, seed + 2)


# ------------------------------------------------------------------------------------------------ 1, 2: the restatements and the table
@pytest.mark.parametrize("name", list(LISTS))
def test_restatements_and_library_agree_on_the_table(P, oracle, name):
    ptr, keep = LISTS[name](oracle)
    rest = S.Restatement(ptr, keep)
    n_tri, n_sph, tri, sph, total = rest.table()
    tab = R.table(tri[:, :9], sph[:, :4])
    assert np.array_equal(bits(tab.tri), bits(tri)) and np.array_equal(bits(tab.sph), bits(sph)) and tab.total == total
    g = P.Scene(ptr, -1, keepalive=keep)
    assert g.sphere_lights() == (False, 0, 0.0)
    g.set_sphere_light_sampling(True)
    if n_tri:
        g.set_lighting(2)
    assert g.sphere_lights() == (True, n_sph, total)
    got_tri, got_sph = g.light_table()
    assert np.array_equal(bits(got_sph), bits(sph)) and len(got_sph) == n_sph
    if n_tri:
        assert np.array_equal(bits(got_tri), bits(tri))
        assert g.lighting() == (2, n_tri, float(tri[-1, 13]))  # the triangles' own count and area
    # W is the area a point outside sees at most, and the sums run on
    assert np.array_equal(sph[:, 5], (2.0 * R.PI) * (sph[:, 3] * sph[:, 3]))
    assert sph[-1, 6] == total and (np.diff(np.concatenate([tri[:, 13], sph[:, 6]])) > 0.0).all()
    g.close()


def test_triangles_keep_their_bits(P, oracle):
    """the light triangles' records with the option on are the ones light_table_build gives without it"""
    ptr, keep = _mixed(oracle)
    off, on = P.Scene(ptr, -1, keepalive=keep), P.Scene(ptr, -1, keepalive=keep)
    off.set_lighting(2)
    on.set_sphere_light_sampling(True)
    on.set_lighting(2)
    a, b = off.light_table()[0], on.light_table()[0]
    assert len(a) == 2 and np.array_equal(bits(a), bits(b))
    assert off.lighting() == on.lighting()
    n, area, table = LS.Restatement(ptr, keep).lights()  # the triangle rule's own restatement
    assert n == 2 and np.array_equal(bits(table), bits(a)) and area == a[-1, 13]
    # either order of the two setters gives the same joined table
    late = P.Scene(ptr, -1, keepalive=keep)
    late.set_lighting(2)
    late.set_sphere_light_sampling(True)
    assert all(np.array_equal(bits(x), bits(y)) for x, y in zip(late.light_table(), on.light_table()))
    for g in (off, on, late):
        g.close()


@pytest.mark.parametrize("name", list(LISTS))
def test_restatements_agree_on_sample_and_pd(oracle, name):
    ptr, keep = LISTS[name](oracle)
    rest = S.Restatement(ptr, keep)
    tab = _numpy_table(rest)
    n = 1 << 16
    p, uv, dirs = _points_and_dirs(tab, n, 21)
    want_d, want_k = rest.sample(p, uv)
    got_d, got_k = R.sample(tab, p, uv)
    assert np.array_equal(got_k, want_k)
    assert int((bits(got_d) != bits(want_d)).any(axis=1).sum()) == 0
    assert len(np.unique(want_k)) == len(tab.cum)  # every entry was drawn
    for probe in (dirs, want_d):
        assert int((bits(R.pd(tab, p, probe)) != bits(rest.pd(p, probe))).sum()) == 0


def test_fma_is_one_rounding():
    rng = np.random.default_rng(8)
    n = 4000
    a, b = rng.normal(size=n) * 2.0 ** rng.integers(-40, 40, n), rng.normal(size=n) * 2.0 ** rng.integers(-40, 40, n)
    c = -(a * b) * (1.0 + rng.integers(-3, 4, n) * 2.0 ** -52)  # near cancellation: where a * b + c rounds twice
    c[::7] = rng.normal(size=len(c[::7]))
    a[:4], b[:4], c[:4] = [0.0, -0.0, 5e-324, 1e300], [3.0, 2.0, 0.5, 1e300], [-0.0, 0.0, 5e-324, -np.inf]
    got = R.fma(a, b, c)
    with np.errstate(all="ignore"):
        want = np.array([R._fma_exact(x, y, z) if np.isfinite([x, y, z]).all() and x != 0.0 and y != 0.0 else x * y + z for x, y, z in zip(a, b, c)])
    assert np.array_equal(bits(got), bits(want))
    with np.errstate(all="ignore"):
        assert (got != a * b + c).any()


# ------------------------------------------------------------------------------------------------ 3: the pd is a density
def _density_points(tab):
    c, r = tab.sph[0, :3], tab.sph[0, 3]
    e = np.array([0.6, 0.0, 0.8])
    return {"outside": c + 4.0 * r * e, "far": c + 40.0 * e, "inside": c + 0.5 * r * e, "centre": c.copy(), "on": c + np.array([r, 0.0, 0.0])}


@pytest.mark.parametrize("name", ["mixed", "one sphere"])
def test_the_pd_is_a_density(oracle, name):
    ptr, keep = LISTS[name](oracle) if name == "mixed" else S.with_spheres(oracle.desc_shirley(32, 16, no_simd=True), [(0.5, 1.0, -6.0, 0.8, 5.0, 1.0)])
    if name != "mixed":
        ptr, keep = C.pointer(ptr), (ptr, keep)
    rest = S.Restatement(ptr, keep)
    tab = _numpy_table(rest)
    n = 1 << 18
    dirs = ES.uniform_directions(n, 31)
    for where, p in _density_points(tab).items():
        if where == "far" and name == "mixed":
            continue  # (outside the box the ceiling is a sliver: nothing a uniform direction finds)
        pd = rest.pd(np.tile(p, (n, 1)), dirs)
        mean, se = 4.0 * np.pi * pd.mean(), 4.0 * np.pi * pd.std(ddof=1) / np.sqrt(n)
        # (inside a lone lamp the pd is one constant and se is 0: what is left is the rounding of a sum of n terms, below n * 2^-53)
        print(f"{name} {where}: 4 pi mean(pd) = {mean:.6f}, se {se:.6f}, z {(mean - 1.0) / max(se, 1e-300):+.2f}")
        assert abs(mean - 1.0) <= 4.0 * se + n * 2.0 ** -53, (name, where, mean, se)


@pytest.mark.parametrize("name", list(LISTS))
def test_every_sampled_direction_has_a_positive_pd(oracle, name):
    ptr, keep = LISTS[name](oracle)
    rest = S.Restatement(ptr, keep)
    tab = _numpy_table(rest)
    n = 1 << 16
    p, uv, _ = _points_and_dirs(tab, n, 33)
    uv = np.random.default_rng(34).uniform(0.0, 1.0, (n, 2)) * [0.5, 1.0]
    d, k = rest.sample(p, uv)
    pd = rest.pd(p, d)
    assert np.isfinite(d).all() and np.isfinite(pd).all() and (pd >= 0.0).all()
    x = (2.0 * uv[:, 0]) * tab.total
    before = np.where(k > 0, tab.cum[np.maximum(k - 1, 0)], 0.0)
    u2 = np.minimum((x - before) / np.concatenate([tab.tri[:, 12], tab.sph[:, 5]])[k], 1.0)
    zero = pd == 0.0
    print(f"{name}: {int(zero.sum())} of {n} sampled directions have pd = 0, {int((u2 == 1.0).sum())} have u2 = 1")
    assert int((zero & (u2 < 1.0)).sum()) == 0 and int(zero.sum()) <= 1


# ------------------------------------------------------------------------------------------------ 4: the closed form
PLANE = dict(w=32, h=16, spp=96, albedo=0.7, depth=5.0)
ONE_LAMP = [(0.0, 2.6, -3.0, 0.3, 30.0)]
TWO_LAMPS = [(0.0, 2.6, -3.0, 0.3, 30.0), (-3.4, 0.0, -2.5, 0.15, 60.0)]


def _closed_form(oracle, lamps, xs, ys, ps):
    """albedo * L * (r^2 / d^2) * cos(theta) per lamp at every sample's own first hit point on the plane"""
    w, h, spp, D = PLANE["w"], PLANE["h"], PLANE["spp"], PLANE["depth"]
    off = ys * w + xs + ps * spp
    dim = 2 + 2 * 2
    dx, dy = oracle.lds_get_vec(dim, off, np.zeros_like(off)), oracle.lds_get_vec(dim, off, np.ones_like(off))
    cx, cy = (xs + dx) * (1.0 / w), 1.0 - (ys + dy) * (1.0 / h)
    p = np.stack([(-1.0 + 2.0 * cx) * D, (-0.5 + 1.0 * cy) * D, np.full(len(xs), -D)], axis=1)
    out = np.zeros(len(xs))
    for x, y, z, r, emit in lamps:
        f = np.array([x, y, z]) - p
        d2 = (f * f).sum(axis=1)
        assert (f[:, 2] > r).all()  # wholly above the plane's horizon
        out += PLANE["albedo"] * emit * (r * r / d2) * (f[:, 2] / np.sqrt(d2))
    return out


@pytest.mark.parametrize("lamps", [ONE_LAMP, TWO_LAMPS], ids=["one lamp", "two lamps"])
def test_a_plane_under_sphere_lamps_converges_to_the_closed_form(oracle, lamps):
    w, h, spp = PLANE["w"], PLANE["h"], PLANE["spp"]
    d, keep = S.plane_scene(lamps, PLANE["albedo"], PLANE["depth"])
    rest = S.Restatement(C.pointer(d), (d, keep))
    xs, ys, ps = LS.all_samples(w, h, spp)
    want = _closed_form(oracle, lamps, xs, ys, ps)

    def z_of(mutant):
        got = rest.trace_samples(2, True, w, h, spp, 2, xs, ys, ps, mutant=mutant)
        assert np.array_equal(got[:, 0], got[:, 1]) and np.array_equal(got[:, 0], got[:, 2])  # (grey scene)
        diff = got[:, 0] - want
        return diff.mean() / (diff.std(ddof=1) / np.sqrt(len(diff))), got[:, 0].mean()

    z, mean = z_of(0)
    print(f"{len(lamps)} lamp(s): frame mean {mean:.6f}, closed form {want.mean():.6f}, z {z:+.2f}")
    assert want.mean() > 0.0 and abs(z) <= 4.0
    wrong = {"4 pi used for 2 pi q": 2}
    if len(lamps) == 2:
        wrong["pd without W_k / W_total"] = 1
    for what, mutant in wrong.items():
        zm, mm = z_of(mutant)
        print(f"  {what}: frame mean {mm:.6f}, z {zm:+.2f}")
        assert abs(zm) > 4.0, what


# ------------------------------------------------------------------------------------------------ 5, 6: the same mean, less variance
def _frames(oracle, name, w, h, spp, lamp_r=S.LAMP_R):
    ptr, keep, _, _, _ = S.descs(name, w, h, lamp_r=lamp_r)
    rest = S.Restatement(ptr, keep)
    xs, ys, ps = LS.all_samples(w, h, spp)
    return [LS.frame_stats(rest.trace_samples(mode, mode == 2, w, h, spp, 8, xs, ys, ps), w * h, spp) for mode in (1, 2)]


@pytest.mark.parametrize("name", ["shirley", "cornell"])
def test_modes_1_and_2_estimate_the_same_mean(oracle, name):
    (m1, se1, _), (m2, se2, _) = _frames(oracle, name, 96, 48, 16)
    z = (m2 - m1) / np.hypot(se1, se2)
    print(f"{name}: mode 1 mean {m1:.6f} (se {se1:.6f}), mode 2 mean {m2:.6f} (se {se2:.6f}), z {z:+.2f}")
    assert m1 > 0.0 and abs(z) <= 4.0


def test_sampling_lowers_the_variance_on_a_small_lamp(oracle):
    (_, _, v1), (_, _, v2) = _frames(oracle, "shirley", 96, 48, 16, lamp_r=0.1)
    ratio = float(v1.sum() / v2.sum())
    both = (v1 > 0.0) & (v2 > 0.0)
    median = float(np.median(v1[both] / v2[both]))
    print(f"small lamp: summed per-pixel variance mode 1 / mode 2 = {ratio:.2f}, median per-pixel ratio {median:.2f}")
    assert ratio > 1.0


# ------------------------------------------------------------------------------------------------ 7: refusals
def test_refusals_keep_the_previous_state(P, oracle):
    L = P.lib()
    # no emissive sphere: refused, the count named; mode 2 keeps refusing with the old message
    d = oracle.desc_shirley(32, 16)
    g = P.Scene(d.ptr, -1, keepalive=d)
    assert L.ptx_scene_set_sphere_light_sampling(g._h, 1) == -1 and "has 0" in P.last_error()
    assert g.sphere_lights() == (False, 0, 0.0)
    assert L.ptx_scene_set_lighting(g._h, 2) == -1 and P.last_error() == OLD_MESSAGE
    assert L.ptx_scene_set_sphere_light_sampling(g._h, 0) == 0  # off on a scene that is off: nothing to do
    g.close()
    # 65 emissive spheres: refused, the count named; 64 are taken
    for n, ok in ((65, False), (64, True)):
        ptr, keep = _spheres_only(oracle, n)
        g = P.Scene(ptr, -1, keepalive=keep)
        rc = L.ptx_scene_set_sphere_light_sampling(g._h, 1)
        assert rc == (0 if ok else -1)
        if not ok:
            assert "65 emissive tree spheres" in P.last_error() and "PTX_MAX_LIGHT_SPHERES = 64" in P.last_error()
            assert g.sphere_lights() == (False, 0, 0.0)
            assert L.ptx_scene_set_lighting(g._h, 2) == -1 and P.last_error() == OLD_MESSAGE
        else:
            assert g.sphere_lights()[:2] == (True, 64)
        g.close()
    # with the option off an emissive sphere is not a reason to accept mode 2: the old message verbatim
    ptr, keep = _spheres_only(oracle, 1)
    g = P.Scene(ptr, -1, keepalive=keep)
    assert L.ptx_scene_set_lighting(g._h, 2) == -1 and P.last_error() == OLD_MESSAGE
    g.set_sphere_light_sampling(True)
    g.set_lighting(2)  # accepted: the light half is the sphere alone
    assert g.lighting() == (2, 0, 0.0) and g.sphere_lights()[:2] == (True, 1)
    # off while mode 2 has nothing else to sample: refused, nothing changes
    assert L.ptx_scene_set_sphere_light_sampling(g._h, 0) == -3 and "set another lighting mode first" in P.last_error()
    assert g.sphere_lights()[:2] == (True, 1) and g.lighting()[0] == 2
    g.set_lighting(1)
    g.set_sphere_light_sampling(False)
    assert g.sphere_lights() == (False, 0, 0.0)
    assert L.ptx_scene_set_lighting(g._h, 2) == -1 and P.last_error() == OLD_MESSAGE
    assert L.ptx_scene_set_sphere_light_sampling(None, 1) == -1
    # the device diagnostics have no CPU fallback
    out = np.zeros(3)
    assert L.ptx_light_pdf(g._h, 1, S._dp(out), S._dp(out), S._dp(out)) == -3
    g.close()


def test_symbols_are_declared_exported_and_mirrored(P):
    header = open(os.path.join(ROOT, "include", "ptx.h")).read()
    names = ("ptx_scene_set_sphere_light_sampling", "ptx_scene_sphere_lights", "ptx_light_table", "ptx_light_sample", "ptx_light_pdf")
    for name in names:
        assert f"int32_t {name}(" in header and name in P.EXPORTS and hasattr(P.lib(), name), name
    assert "#define PTX_MAX_LIGHT_SPHERES 64" in header and P.lib().ptx_version() == 6
    for method in ("set_sphere_light_sampling", "sphere_lights", "light_table", "light_sample", "light_pdf"):
        assert callable(getattr(P.Scene, method))
    import inspect
    from path_tracer_ocaml_amd.integrator import Integrator
    assert "sphere_light_sampling" in inspect.signature(Integrator.create).parameters
