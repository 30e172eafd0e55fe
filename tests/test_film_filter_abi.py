"""The film at any order and radius at the C ABI, without a GPU: ptx_film_weights against the oracle's orc_filter_binomial and the
Fraction restatement (tests/film_reference.py) bit for bit on every accepted (order, radius); the refusals; the sticky film of a
host-only scene; and the gather rule against the reference's splat (Film_tile.write_pixel + stitch_tile) within a derived bound."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

import film_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("ptx_film_defaults", "ptx_film_weights", "ptx_scene_set_film", "ptx_scene_film", "ptx_film_resolve_ex_device",
       "ptx_film_resolve_banded_ex_device", "ptx_film_resolve_counts_ex_device")
ERR_ARG, ERR_STATE = -1, -3


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _weights(L, abi, order, radius, flags=0, reserved=0, want2d=True):
    n = 2 * radius + 1 if 0 <= radius <= 7 else 1
    f = abi.FilmParams(order, radius, flags, reserved)
    w1, w2 = np.full(n, -1.0), np.full((n, n), -1.0)
    rc = L.ptx_film_weights(C.byref(f), w1.ctypes.data_as(abi.c_double_p), w2.ctypes.data_as(abi.c_double_p) if want2d else None)
    return rc, w1, w2


def test_new_entry_points_are_declared_exported_and_listed():
    import path_tracer_ocaml_amd as P
    hdr = open(os.path.join(ROOT, "include", "ptx.h")).read()
    L = P.lib()
    for name in NEW:
        assert f"{name}(" in hdr, name
        assert hasattr(L, name), name
        assert name in P.EXPORTS, name
        assert getattr(L, name).argtypes, name
    for line in ("#define PTX_FILM_MAX_ORDER 16", "#define PTX_FILM_MAX_RADIUS 7", "#define PTX_FILM_RENORMALISE 1",
                 "#define PTX_ABI_VERSION 6"):
        assert line in hdr, line
    assert L.ptx_version() == 6
    assert callable(P.film_defaults) and callable(P.film_weights) and callable(P.Scene.set_film) and callable(P.Scene.film)


def test_film_params_layout_matches_c(tmp_path):
    from path_tracer_ocaml_amd import abi
    fields = ("order", "pixel_radius", "flags", "reserved")
    src = tmp_path / "fp.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "ptx.h"\nint main(void){'
                   'printf("%zu %zu", sizeof(ptx_film_params), _Alignof(ptx_film_params));'
                   + "".join(f'printf(" %zu", offsetof(ptx_film_params, {f}));' for f in fields)
                   + 'printf(" %d %d %d\\n", PTX_FILM_MAX_ORDER, PTX_FILM_MAX_RADIUS, PTX_FILM_RENORMALISE);return 0;}\n')
    exe = tmp_path / "fp"
    subprocess.check_call(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    T = abi.FilmParams
    assert got == [C.sizeof(T), C.alignment(T)] + [getattr(T, f).offset for f in fields] + [abi.PTX_FILM_MAX_ORDER,
                                                                                              abi.PTX_FILM_MAX_RADIUS,
                                                                                              abi.PTX_FILM_RENORMALISE]
    assert got[:6] == [16, 4, 0, 4, 8, 12]


def test_weights_equal_the_oracle_and_the_restatement_on_every_accepted_pair(oracle):
    import path_tracer_ocaml_amd as P
    from path_tracer_ocaml_amd import abi
    L, O = P.lib(), oracle.lib()
    pairs = R.accepted_pairs()
    assert len(pairs) == 72
    for order, radius in pairs:
        n = 2 * radius + 1
        rc, w1, w2 = _weights(L, abi, order, radius)
        assert rc == 0, (order, radius, P.last_error())
        o2, o1 = np.zeros((n, n)), np.zeros(n)
        assert O.orc_filter_binomial(order, radius, o2.ctypes.data_as(abi.c_double_p), o1.ctypes.data_as(abi.c_double_p)) == n
        r1, r2 = R.weights(order, radius)
        assert np.array_equal(bits(w1), bits(o1)) and np.array_equal(bits(w2), bits(o2)), (order, radius)
        assert np.array_equal(bits(w1), bits(r1)) and np.array_equal(bits(w2), bits(r2)), (order, radius)
        # what the issue found on this region: positive, palindromic bit for bit, the 2-D weights sum to 1
        assert (w1 > 0).all() and np.array_equal(bits(w1), bits(w1[::-1])), (order, radius)
        assert abs(math.fsum(w2.ravel().tolist()) - 1.0) <= 2.3e-16, (order, radius)
        # the 2-D output is optional
        rc, v1, v2 = _weights(L, abi, order, radius, want2d=False)
        assert rc == 0 and np.array_equal(bits(v1), bits(w1)) and (v2 == -1.0).all()
        p1, p2 = P.film_weights(order, radius)
        assert np.array_equal(bits(p1), bits(w1)) and np.array_equal(bits(p2), bits(w2))


def test_five_one_gives_the_nine_weights_of_the_default_film():
    """binomial_3x3 of csrc/ptx_api.inc, the default path's kernel: taps 11/3, 26/3, 11/3 -> / 3.0, fold, normalise, outer product"""
    import path_tracer_ocaml_amd as P
    from path_tracer_ocaml_amd import abi
    rc, w1, w2 = _weights(P.lib(), abi, 5, 1)
    assert rc == 0
    w = [11.0 / 3.0, 26.0 / 3.0, 11.0 / 3.0]
    total = 0.0
    for v in w:
        total = total + v
    w = [v / total for v in w]
    want = np.array([w[j // 3] * w[j % 3] for j in range(9)])
    assert np.array_equal(bits(w2.ravel()), bits(want))
    assert np.array_equal(bits(w1), bits(w))


@pytest.mark.parametrize("order, radius, flags, reserved, word", [
    (0, 0, 0, 0, "order"), (17, 1, 0, 0, "order"), (5, -1, 0, 0, "pixel_radius"), (16, 8, 0, 0, "pixel_radius"),
    (5, 3, 0, 0, "2 * pixel_radius + 1"), (1, 1, 0, 0, "2 * pixel_radius + 1"), (14, 7, 0, 0, "2 * pixel_radius + 1"),
    (5, 1, 2, 0, "flags"), (5, 1, 3, 0, "flags"), (5, 1, 0, 1, "reserved"),
])
def test_refused_parameters_are_argument_errors_that_name_the_rule(order, radius, flags, reserved, word, oracle):
    import path_tracer_ocaml_amd as P
    from path_tracer_ocaml_amd import abi
    L = P.lib()
    rc, w1, w2 = _weights(L, abi, order, radius, flags, reserved)
    assert rc == ERR_ARG and word in P.last_error(), P.last_error()
    assert (w1 == -1.0).all() and (w2 == -1.0).all()
    d = oracle.desc_shirley(16, 12)
    s = P.Scene(d.ptr, -1, keepalive=d)
    f = abi.FilmParams(order, radius, flags, reserved)
    assert L.ptx_scene_set_film(s._h, C.byref(f)) == ERR_ARG and word in P.last_error()
    assert s.film() == (5, 1, False)
    # the device entry points check the film before they touch a device (the buffers here are never read)
    buf = np.zeros(16 * 12 * 3)
    n = np.ones(16 * 12, dtype=np.int32)
    p, q = buf.ctypes.data, n.ctypes.data
    assert L.ptx_film_resolve_ex_device(0, 16, 12, 1, C.byref(f), p, p, None) == ERR_ARG and word in P.last_error()
    assert L.ptx_film_resolve_banded_ex_device(0, 16, 12, 1, C.byref(f), p, 1, 8, 16, p, None) == ERR_ARG and word in P.last_error()
    assert L.ptx_film_resolve_counts_ex_device(0, 16, 12, C.byref(f), p, q, p, None) == ERR_ARG and word in P.last_error()
    s.close()


def test_null_pointers_are_argument_errors():
    import path_tracer_ocaml_amd as P
    from path_tracer_ocaml_amd import abi
    L = P.lib()
    f = abi.FilmParams(5, 1, 0, 0)
    w = np.zeros(3)
    assert L.ptx_film_defaults(None) == ERR_ARG
    assert L.ptx_film_weights(None, w.ctypes.data_as(abi.c_double_p), None) == ERR_ARG
    assert L.ptx_film_weights(C.byref(f), None, None) == ERR_ARG
    assert L.ptx_scene_set_film(None, C.byref(f)) == ERR_ARG
    assert L.ptx_scene_film(None, C.byref(f)) == ERR_ARG
    assert L.ptx_film_resolve_ex_device(0, 4, 4, 1, C.byref(f), None, None, None) == ERR_ARG
    assert L.ptx_film_resolve_banded_ex_device(0, 4, 4, 1, C.byref(f), None, 1, 8, 4, None, None) == ERR_ARG
    assert L.ptx_film_resolve_counts_ex_device(0, 4, 4, C.byref(f), None, None, None, None) == ERR_ARG
    assert L.ptx_film_resolve_counts_ex_device(-1, 4, 4, C.byref(f), None, None, None, None) == ERR_STATE


def test_a_host_only_scene_keeps_its_film(oracle):
    import path_tracer_ocaml_amd as P
    from path_tracer_ocaml_amd import abi
    assert P.film_defaults() == (5, 1, False)
    d = oracle.desc_shirley(16, 12)
    s = P.Scene(d.ptr, -1, keepalive=d)
    assert s.film() == (5, 1, False)
    s.set_film(7, 3)
    assert s.film() == (7, 3, False)
    s.set_film(15, 7, renormalise=True)
    assert s.film() == (15, 7, True)
    out = abi.FilmParams()
    assert P.lib().ptx_scene_film(s._h, None) == ERR_ARG
    assert P.lib().ptx_scene_film(s._h, C.byref(out)) == 0 and (out.order, out.pixel_radius, out.flags, out.reserved) == (15, 7, 1, 0)
    assert P.lib().ptx_scene_set_film(s._h, None) == 0  # NULL restores the default
    assert s.film() == (5, 1, False)
    s.set_film(5, 0)
    s.set_film()
    assert s.film() == (5, 1, False)
    with pytest.raises(ValueError, match="lopsided"):
        s.set_film(5, 3)
    with pytest.raises(ValueError, match="order"):
        s.set_film(17, 1)
    assert s.film() == (5, 1, False)
    # a host-only scene still has no CPU fallback, whatever its film
    s.set_film(7, 3)
    with pytest.raises(P.PtxError, match="no CPU fallback"):
        s.render(16, 12, 1, 1)
    s.close()


def test_the_fast_fma_is_the_fraction_fma():
    rng = np.random.default_rng(11)
    a = rng.uniform(0.0, 1.0, 400) * 10.0 ** rng.integers(-8, 1, 400)
    b = rng.uniform(0.0, 10.0, 400) * 10.0 ** rng.integers(-6, 6, 400)
    c = rng.uniform(0.0, 10.0, 400) * 10.0 ** rng.integers(-6, 6, 400)
    b[::7] = 0.0
    c[::5] = 0.0
    for x, y, z in zip(a.tolist(), b.tolist(), c.tolist()):
        assert R.fma(x, y, z) == R.fma_exact(x, y, z)
    # a product whose low half decides the rounding: (1 + 2^-52)^2 = 1 + 2^-51 + 2^-104
    x = 1.0 + 2.0 ** -52
    assert R.fma(x, x, -(1.0 + 2.0 ** -51)) == 2.0 ** -104 == R.fma_exact(x, x, -(1.0 + 2.0 ** -51))


@pytest.mark.parametrize("W,H", [(7, 5), (20, 3)])
@pytest.mark.parametrize("order,radius", [(5, 0), (5, 1), (7, 3), (15, 7)])
def test_gather_agrees_with_the_splat(W, H, order, radius):
    """The rule gathers the raw sums S(q) = the pass-order sum of q's samples; the reference splats every sample.  Both sum the same
    non-negative terms w * c, so each is within (its number of roundings) * 2^-53 of the exact sum, relatively: the splat rounds once
    per term (taps * spp fmas), the gather spp times per raw sum and once per tap, and the weights' own product is shared.  Hence
    |gather - splat| <= 2 * (taps * spp + spp + taps + 4) * 2^-53 relative -- derived, not measured."""
    taps = (2 * radius + 1) ** 2
    for spp in (1, 3, 16):
        rng = np.random.default_rng(1000 * W + 10 * spp + radius)
        samples = rng.uniform(0.0, 4.0, (spp, H, W, 3)) * rng.choice([0.0, 1.0, 1.0, 50.0], (spp, H, W, 1))
        splat = R.splat(samples, order, radius)
        acc, _, _, _ = R.accumulate(R.raw_sums(samples), order, radius)
        bound = 2.0 * (taps * spp + spp + taps + 4) * 2.0 ** -53
        scale = np.maximum(np.abs(splat), np.abs(acc))
        rel = np.where(scale > 0, np.abs(splat - acc) / np.where(scale > 0, scale, 1.0), 0.0)
        assert float(rel.max()) <= bound, (spp, float(rel.max()), bound)
        if spp == 1 and radius == 0:
            assert np.array_equal(bits(splat), bits(acc))


def _cli(*args):
    exe = os.path.join(ROOT, "path_tracer_ocaml_amd", "shirley_spheres")
    env = dict(os.environ)
    env["LD_LIBRARY_PATH"] = "/opt/rocm/lib:" + env.get("LD_LIBRARY_PATH", "")
    return subprocess.run([exe, "--dimension=16,8", "--no-progress", *args], capture_output=True, text=True, env=env, timeout=60)


@pytest.mark.parametrize("args, match", [
    (("--filter=5,3",), "order 5 is smaller than 2 * pixel_radius + 1 = 7"),
    (("--filter=17,1",), "order 17 is outside 1 .. 16"),
    (("--filter=16,8", "--filter-renormalise"), "pixel_radius 8 is outside 0 .. 7"),
    (("--filter=5",), "invalid value for --filter, expected ORDER,RADIUS"),
    (("--filter=5,1,0",), "invalid value for --filter, expected ORDER,RADIUS"),
])
def test_cli_refuses_a_bad_filter_before_anything_is_rendered(args, match, tmp_path):
    out = tmp_path / "never.png"
    r = _cli(*args, "-o", str(out))
    assert r.returncode == 124, (r.returncode, r.stderr)
    assert match in r.stderr
    assert r.stdout == "" and not out.exists()


def test_cli_usage_lists_the_filter_flags():
    r = _cli("--help")
    assert r.returncode == 0
    assert "--filter=ORDER,RADIUS" in r.stderr and "--filter-renormalise" in r.stderr


def test_ocaml_binding_exposes_the_film():
    b = os.path.join(ROOT, "bindings", "ocaml")
    ml = open(os.path.join(b, "ptx.ml")).read()
    for name in ("let set_film", "let film ", "let film_weights", '"ptx_ml_set_film_stub"', '"ptx_ml_film_stub"', '"ptx_ml_film_weights_stub"'):
        assert name in ml, name
    c = open(os.path.join(b, "ptx_stubs.c")).read()
    for name in ("ptx_ml_set_film_stub", "ptx_ml_film_stub", "ptx_ml_film_weights_stub"):
        assert f"CAMLprim value {name}(" in c, name
    m = open(os.path.join(b, "ptx_ml_marshal.h")).read()
    assert "ptx_scene_set_film(" in m and "ptx_film_weights(" in m


def test_python_layers_take_a_film():
    import inspect
    import path_tracer_ocaml_amd as P
    from path_tracer_ocaml_amd import abi, distributed, integrator
    for fn in (P.film_resolve_device, P.film_resolve_banded_device, P.film_resolve_counts_device, integrator.Integrator.create,
               distributed.BandGather.film):
        assert "film" in inspect.signature(fn).parameters, fn
    assert (abi.film_params().order, abi.film_params().pixel_radius, abi.film_params().flags) == (5, 1, 0)
    f = abi.film_params((7, 3, True))
    assert (f.order, f.pixel_radius, f.flags, f.reserved) == (7, 3, 1, 0)
    for bad in ((5, 3), (0, 0), (17, 1), (5, -1), (16, 8), (5,)):
        with pytest.raises(ValueError):
            abi.film_params(bad)
    with pytest.raises(ValueError, match="wait"):
        P.film_resolve_banded_device(0, 4, 4, 1, 0, 1, 8, 4, 0, wait=False, film=(7, 3))
