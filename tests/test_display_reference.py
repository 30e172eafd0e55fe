"""The display rule on the host, without a GPU: ptx_display_apply against the numpy restatement (tests/display_reference.py) bit for
bit on images made of the values where the rule can go wrong, under every accepted setting; the sRGB thresholds against mpmath; the
default display against the PNG writer's rows; every refusal."""
import ctypes as C

import numpy as np
import pytest

import display_reference as R

ERR_ARG, ERR_STATE = -1, -3


@pytest.fixture(scope="module")
def P():
    import path_tracer_ocaml_amd as P
    P.lib()
    return P


@pytest.fixture(scope="module")
def T(P):
    return P.display_thresholds()


def test_thresholds_are_strictly_increasing_and_inside_the_unit_interval(T):
    assert T.shape == (255,) and T.dtype == np.float64
    assert np.all(np.diff(T) > 0.0)
    assert 0.0 < T[0] and T[-1] < 1.0


def test_thresholds_are_the_header_formula_within_8_ulp_of_mpmath(T):
    """at most 2 ulp on the base after e, the add and the divide, times the exponent 2.4, plus libm's pow at under 1 ulp"""
    mp = pytest.importorskip("mpmath")
    mp.mp.dps = 100
    worst = 0.0
    for k in range(1, 256):
        e = (mp.mpf(k) - mp.mpf("0.5")) / 255
        exact = e / mp.mpf("12.92") if e <= mp.mpf("0.04045") else ((e + mp.mpf("0.055")) / mp.mpf("1.055")) ** mp.mpf("2.4")
        got = float(T[k - 1])
        ulp = float(np.spacing(got))
        worst = max(worst, abs(float((mp.mpf(got) - exact) / ulp)))
        # and each threshold separates the codes it is meant to separate: encode(T[k]) * 255 is k - 0.5 within 1e-9
        enc = 12.92 * got if got <= 0.0031308 else 1.055 * got ** (1 / 2.4) - 0.055
        assert abs(enc * 255.0 - (k - 0.5)) < 1e-9, k
    print("worst threshold error, ulp:", worst)
    assert worst <= 8.0


def test_thresholds_handed_out_are_the_ones_apply_searches(P, T):
    """v whose square is T[k], or one of its two neighbours, exactly: the code steps from k - 1 to k AT the threshold, not after it"""
    k = np.arange(1, 256)
    lo, hi = np.nextafter(T, -np.inf), np.nextafter(T, np.inf)
    v = np.sqrt(np.stack([lo, T, hi], axis=-1))
    L = v * v
    code = P.display_apply(v, transfer="srgb", tone="none", exposure=1.0).astype(np.int64)
    hit = 0
    for col, want in ((0, k - 1), (1, k), (2, k)):
        exact = L[:, col] == (lo, T, hi)[col]  # the square landed on the value meant
        hit += int(exact.sum())
        assert np.array_equal(code[exact, col], want[exact]), col
    assert hit > 255, "too few exact squares to show anything"
    assert np.array_equal(code, np.searchsorted(T, L, side="right"))


@pytest.mark.parametrize("fmt, transfer, tone, exposure", R.settings())
def test_apply_equals_the_restatement_on_edge_values(P, T, fmt, transfer, tone, exposure):
    img = R.full_edge_image(T)
    got = P.display_apply(img, format=fmt, transfer=transfer, tone=tone, exposure=exposure)
    want = R.apply(img, T, fmt, transfer, tone, exposure)
    assert got.dtype == want.dtype and got.shape == want.shape
    assert R.same(got, want), np.argwhere(got != want)[:8]
    if fmt.startswith("rgba"):
        assert np.all(got[..., 3] == (255 if fmt == "rgba8" else 1.0))


def test_edge_values_reach_the_cases_they_are_meant_for(T):
    v = R.edge_values(T)
    tiny = np.finfo(np.float32).tiny
    with np.errstate(all="ignore"):
        f = v.astype(np.float32)
        assert np.any((np.abs(f) > 0) & (np.abs(f) < tiny)), "binary32 subnormal results"
        assert np.any((v != 0) & (f == 0)), "results that round to zero"
        assert np.any(np.isnan(v)) and np.any(np.isposinf(v)) and np.any(np.isneginf(v)) and np.any(v < 0)
        L = v * v
        for e in R.EXPOSURES[1:]:
            assert np.any(L * e > R.CAP) and np.any(L * e == R.CAP) and np.any((L * e < R.CAP) & (L * e > R.CAP / 2)), e
    for k in range(256):
        assert k / 255.0 in v
    assert np.all(np.isin(T, v))


@pytest.mark.parametrize("n", [0, 1, 2, 3, 4, 5, 63, 64, 65, 257, 13 * 11])
def test_apply_at_odd_sizes_writes_exactly_its_pixels(P, T, n):
    from path_tracer_ocaml_amd import abi
    img = R.edge_image(T, n, seed=n)
    for fmt in R.FORMATS:
        d = abi.display_params(None, fmt, "linear", "aces", 0.25)
        b = P.display_pixel_bytes(fmt)
        out = np.full(n * b + 16, 0xA5, dtype=np.uint8)
        assert P.lib().ptx_display_apply(C.byref(d), n, img.ctypes.data_as(abi.c_double_p), C.c_void_p(out.ctypes.data)) == 0
        assert np.all(out[n * b:] == 0xA5)
        dtype, ch = abi.PTX_PIXEL_LAYOUT[d.format]
        got = out[:n * b].view(dtype).reshape(n, ch)
        assert R.same(got, R.apply(img, T, fmt, "linear", "aces", 0.25))


def test_default_display_is_the_png_writers_rows(P, T, tmp_path):
    Image = pytest.importorskip("PIL.Image")
    from path_tracer_ocaml_amd import host as H
    vals = R.edge_values(T)
    vals = vals[np.isfinite(vals)]  # (the writer takes what a render can produce; NaN and inf are checked against the rule above)
    h, w = 31, -(-len(vals) // (31 * 3))
    rgb = np.resize(vals, (h, w, 3))
    path = str(tmp_path / "edge.png")
    H.write_png(path, rgb)
    rows = np.array(Image.open(path).convert("RGB"))
    d = P.display_defaults()
    assert (d.format, d.transfer, d.tone, d.flags, d.exposure, list(d.reserved)) == (0, 0, 0, 0, 1.0, [0, 0, 0, 0])
    assert np.array_equal(P.display_apply(rgb, d), rows)
    assert np.array_equal(P.display_apply(rgb), rows)


def test_pixel_bytes(P):
    assert [P.display_pixel_bytes(f) for f in R.FORMATS] == [3, 4, 12, 16]
    assert [P.lib().ptx_display_pixel_bytes(i) for i in range(4)] == [3, 4, 12, 16]
    for bad in (-1, 4, 99):
        assert P.lib().ptx_display_pixel_bytes(bad) == ERR_ARG
        assert "format" in P.last_error()


def _refused(P, message, **fields):
    from path_tracer_ocaml_amd import abi
    d = abi.display_params(None, **{k: v for k, v in fields.items() if k in ("format", "transfer", "tone", "exposure")})
    d.flags = fields.get("flags", 0)
    for i, r in enumerate(fields.get("reserved", ())):
        d.reserved[i] = r
    img = np.full((2, 3), 0.5)
    out = np.full(64, 0xA5, dtype=np.uint8)
    L = P.lib()
    assert L.ptx_display_check(C.byref(d)) == ERR_ARG
    assert P.last_error().startswith("display: ") and message in P.last_error(), P.last_error()
    assert L.ptx_display_apply(C.byref(d), 2, img.ctypes.data_as(abi.c_double_p), C.c_void_p(out.ctypes.data)) == ERR_ARG
    assert message in P.last_error()
    assert np.all(out == 0xA5), "a refused call writes nothing"
    # the device and render entry points refuse the same settings before they look at the device or the scene
    assert L.ptx_display_image_device(0, C.byref(d), 2, None, None, None) == ERR_ARG and message in P.last_error()
    assert L.ptx_render_display(None, None, C.byref(d), C.c_void_p(out.ctypes.data), None, None, None) == ERR_ARG
    assert message in P.last_error()
    assert L.ptx_render_progressive_display(None, None, None, None, C.byref(d), C.c_void_p(out.ctypes.data), None, None, None, None,
                                            None) == ERR_ARG
    assert message in P.last_error()
    assert np.all(out == 0xA5)


@pytest.mark.parametrize("message, fields", [
    ("unknown format", dict(format=4)), ("unknown format", dict(format=-1)),
    ("unknown transfer", dict(transfer=3)), ("unknown transfer", dict(transfer=-1)),
    ("unknown tone", dict(tone=3, transfer=1)), ("unknown tone", dict(tone=-1, transfer=1)),
    ("flags must be 0", dict(flags=1)),
    ("reserved[0] must be 0", dict(reserved=(1,))), ("reserved[3] must be 0", dict(reserved=(0, 0, 0, 7))),
    ("exposure must be finite and >= 0", dict(transfer=1, exposure=float("nan"))),
    ("exposure must be finite and >= 0", dict(transfer=1, exposure=float("inf"))),
    ("exposure must be finite and >= 0", dict(transfer=1, exposure=-1.0)),
    ("exposure must be finite and >= 0", dict(transfer=2, exposure=-0.5)),
    ("PTX_TRANSFER_REFERENCE needs tone PTX_TONE_NONE and exposure 1.0", dict(transfer=0, tone=1)),
    ("PTX_TRANSFER_REFERENCE needs tone PTX_TONE_NONE and exposure 1.0", dict(transfer=0, tone=2)),
    ("PTX_TRANSFER_REFERENCE needs tone PTX_TONE_NONE and exposure 1.0", dict(transfer=0, exposure=2.0)),
    ("PTX_TRANSFER_REFERENCE needs tone PTX_TONE_NONE and exposure 1.0", dict(transfer=0, exposure=0.0)),
    ("binary32 formats carry linear or reference values", dict(format=2, transfer=2)),
    ("binary32 formats carry linear or reference values", dict(format=3, transfer=2, tone=2, exposure=0.25)),
])
def test_refusals_name_the_rule_and_write_nothing(P, message, fields):
    _refused(P, message, **fields)


def test_null_arguments_and_sizes(P):
    from path_tracer_ocaml_amd import abi
    L = P.lib()
    d = P.display_defaults()
    img, out = np.zeros(3), np.zeros(3, dtype=np.uint8)
    dp = abi.c_double_p
    assert L.ptx_display_defaults(None) == ERR_ARG
    assert L.ptx_display_check(None) == ERR_ARG
    assert L.ptx_display_thresholds(None) == ERR_ARG
    assert L.ptx_display_apply(None, 1, img.ctypes.data_as(dp), C.c_void_p(out.ctypes.data)) == ERR_ARG
    assert L.ptx_display_apply(C.byref(d), -1, img.ctypes.data_as(dp), C.c_void_p(out.ctypes.data)) == ERR_ARG
    assert L.ptx_display_apply(C.byref(d), 1, None, C.c_void_p(out.ctypes.data)) == ERR_ARG
    assert L.ptx_display_apply(C.byref(d), 1, img.ctypes.data_as(dp), None) == ERR_ARG
    assert L.ptx_display_apply(C.byref(d), 0, None, None) == 0
    assert L.ptx_display_image_device(-1, C.byref(d), 1, C.c_void_p(16), C.c_void_p(32), None) == ERR_STATE
    assert L.ptx_display_image_device(0, C.byref(d), -1, C.c_void_p(16), C.c_void_p(32), None) == ERR_ARG
    assert L.ptx_display_image_device(0, C.byref(d), 1, C.c_void_p(16), C.c_void_p(36), None) == ERR_ARG
    assert "16-byte aligned" in P.last_error()
    # a host-only scene pins nothing and renders nothing
    assert L.ptx_image_pin_bytes(None, C.c_void_p(out.ctypes.data), 3) == ERR_ARG


def test_python_names_and_shapes(P, T):
    img = np.linspace(0.0, 1.2, 5 * 7 * 3).reshape(5, 7, 3)
    for fmt, (dtype, ch) in zip(R.FORMATS, (("uint8", 3), ("uint8", 4), ("float32", 3), ("float32", 4))):
        got = P.display_apply(img, format=fmt, transfer="linear", tone="reinhard", exposure=2.0)
        assert got.shape == (5, 7, ch) and got.dtype == np.dtype(dtype)
        assert R.same(got, R.apply(img, T, fmt, "linear", "reinhard", 2.0))
    with pytest.raises(ValueError):
        P.display_apply(img, transfer="gamma")
    with pytest.raises(P.PtxError, match="binary32 formats"):
        P.display_apply(img, format="rgb32f", transfer="srgb")
