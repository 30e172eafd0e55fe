"""The oracle's shading against an oracle-independent restatement of the reference's rules in interval arithmetic
(tests/exact_shading.py): the state after the first scatter (orc_debug_first_scatter) and the radiance of every sample
at max_bounces 0, 1 and 2 (orc_trace_samples), on the stock scenes, shading soups and families of primitives placed
so that a decision sits at its boundary: the top pole test (first hits), the bottom pole test (second hits, after a
mirror), checker parity, TIR, Schlick against u, and the scatter side of metal's absorb rule (its absorb side cannot
be robust for a hit from outside, where omega_r.z > 0 exactly).  The families run at max_bounces 2 only (the camera rays they are solved on are those of that depth).
A mutation self-test proves the comparison can fail."""
import ctypes as C

import numpy as np
import pytest

import exact_shading as S

_CACHE = {}


def first_scatter(oracle, sc, W, H, spp, mb, xs, ys, ps):
    """orc_debug_first_scatter: next ray (n, 6), attenuation (n, 3), alive (n,), info (n, 3) = prim, material, scatter kind."""
    n = len(xs)
    ip, dp = oracle.ip, oracle.dp
    L = oracle.lib()
    L.orc_debug_first_scatter.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int64, ip, ip, ip, dp, dp, ip, ip]
    ray, att, alive, info = np.zeros((n, 6)), np.zeros((n, 3)), np.zeros(n, np.int32), np.zeros((n, 3), np.int32)
    xs, ys, ps = (np.ascontiguousarray(a, dtype=np.int32) for a in (xs, ys, ps))
    L.orc_debug_first_scatter(sc._h, W, H, spp, mb, n, xs.ctypes.data_as(ip), ys.ctypes.data_as(ip), ps.ctypes.data_as(ip),
                              ray.ctypes.data_as(dp), att.ctypes.data_as(dp), alive.ctypes.data_as(ip), info.ctypes.data_as(ip))
    return ray, att, alive, info


def case(name, oracle, mb=2):
    """Everything a scene needs, built once per module: the description, its tables, the samples through the
    restatement at max_bounces mb, and the oracle's first scatter and radiance of those samples."""
    key = (name, mb)
    if key in _CACHE:
        return _CACHE[key]
    from path_tracer_ocaml_amd import abi
    if name in S.FAMILIES:
        ptr, keep, W, H, spp, xs, ys, ps = S.family_desc(name, oracle, abi)
    else:
        ptr, keep, W, H, spp = S.stock_desc(name, oracle, abi)
        xs, ys, ps = S.random_samples(name, W, H, spp)
    tab = S.Tables(ptr)
    smp = S.Samples(oracle, tab, W, H, spp, mb, xs, ys, ps)
    sc = oracle.Scene(ptr, keep)
    fs = first_scatter(oracle, sc, W, H, spp, max(mb, 2), xs, ys, ps) if mb == 2 else None
    rgb, _ = sc.trace_samples(W, H, spp, mb, xs, ys, ps)
    _CACHE[key] = (ptr, keep, smp, fs, rgb)
    return _CACHE[key]


SCENES = S.STOCK + list(S.FAMILIES)


@pytest.mark.slow
@pytest.mark.parametrize("name", SCENES)
def test_first_scatter_equals_restatement(name, oracle):
    """The winner, the material and scatter kind, alive, the next ray and the attenuation of every robust sample."""
    ptr, keep, smp, (ray, att, alive, info), rgb = case(name, oracle)
    bad, summ, dec, s = S.check_first_scatter(smp, ray, att, alive, info)
    rob = dec.robust & smp.camera_ok
    first_target = name in S.FAMILIES and not S.FAMILIES[name].endswith("_2")
    if first_target:
        summ["near_" + S.FAMILIES[name]] = S.near_count(dec, S.FAMILIES[name], rob)
    print(f"\n{name}: {summ}")
    assert not bad, "\n".join(bad)
    assert summ["camera_outside"] == 0, "orc_camera_ray lies outside the restated camera ray"
    tight = S.check_tightness(name, summ)
    assert not tight, "\n".join(tight)
    assert summ["robust"] >= S.MIN_ROBUST * summ["samples"], f"{name}: only {summ['robust']} robust samples"
    if first_target:
        near = summ["near_" + S.FAMILIES[name]]
        assert near >= S.MIN_NEAR * summ["samples"], f"{name}: only {near} samples within 100 half-widths of the target"


RADIANCE_CASES = [(n, mb) for n in S.STOCK for mb in (0, 1, 2)] + [(n, S.FAMILY_MB) for n in S.FAMILIES]


@pytest.mark.slow
@pytest.mark.parametrize("name,mb", RADIANCE_CASES)
def test_radiance_equals_restatement(name, mb, oracle):
    """orc_trace_samples at max_bounces mb.  For 2 the second segment starts from the oracle's binary64 next ray, which
    must first lie inside the first scatter's enclosure (a chain on verified binary64 states)."""
    ptr, keep, smp, fs, rgb = case(name, oracle, mb)
    if mb == 2:
        ray, att, alive, info = fs
        bad, _, _, _ = S.check_first_scatter(smp, ray, att, alive, info)
        assert not bad, "\n".join(bad)
        target = S.FAMILIES.get(name, "")
        target = target if target.endswith("_2") else None
        bad, summ, rob = S.check_radiance(smp, rgb, ray[:, :3], ray[:, 3:], target=target)
    else:
        target = None
        bad, summ, rob = S.check_radiance(smp, rgb)
    print(f"\n{name} max_bounces {mb}: {summ}")
    assert not bad, "\n".join(bad)
    assert summ["robust"] >= S.MIN_ROBUST * summ["samples"], f"{name}: only {summ['robust']} robust samples"
    if target is not None:  # a second-segment target: the family's floor is met here
        near = summ["near_" + target]
        assert near >= S.MIN_NEAR * summ["samples"], f"{name}: only {near} samples within 100 half-widths of the target"
    tight = S.check_tightness(name, summ)
    assert not tight, "\n".join(tight)


# the scenes where each wrong rule must show: any robust sample whose oracle result leaves the mutant's enclosure
MUTANT_SCENES = ["shirley", "cornell", "shade_soup-1", "pole", "pole_bottom", "checker_tri", "checker_sph", "tir", "emit_black"]


@pytest.mark.slow
@pytest.mark.parametrize("mutant", S.MUTANTS)
def test_mutants_are_rejected(mutant, oracle):
    """Each deliberately wrong variant of the restatement is rejected by at least one robust sample."""
    rejected = {}
    for name in MUTANT_SCENES:
        ptr, keep, smp, (ray, att, alive, info), rgb = case(name, oracle)
        bad, _, _, _ = S.check_first_scatter(smp, ray, att, alive, info, mut=(mutant,))
        bad2, _, _ = S.check_radiance(smp, rgb, ray[:, :3], ray[:, 3:], mut=(mutant,))
        if bad or bad2:
            rejected[name] = (bad + bad2)[0]
            break
    print(f"\n{mutant}: rejected by {rejected}")
    assert rejected, f"mutant {mutant} passes every scene: the comparison cannot see it"
