"""Display outputs on the GPU, bit for bit: k_display_image against the host's ptx_display_apply on the edge-value images, at sizes
around the kernel's four-pixel quads and its 256-thread workgroups; ptx_render_display and ptx_render_progressive_display against
the display of the f64 entry points' images -- unpinned, pinned through the row-slab pipeline at odd widths and ragged slabs, over
two aliased replicas, with the denoiser; refusals that leave `out` alone; the launched-kernel record unchanged by the display.

Every test calls a symbol the library did not export before the display existed.  (A binary32 NaN counts as equal to a NaN: the
payload of a NaN the arithmetic itself makes differs between the host's and the device's instruction sets; display_reference.same.)"""
import ctypes as C

import numpy as np
import pytest

import display_reference as R

pytestmark = pytest.mark.gpu

SIZES = (1, 2, 3, 4, 5, 63, 64, 65, 257, 13 * 11)
SPP, DEPTH = 3, 2


@pytest.fixture(scope="module")
def P():
    import path_tracer_ocaml_amd as P
    assert P.lib().ptx_device_count() >= 1, P.last_error()
    return P


@pytest.fixture(scope="module")
def torch():
    return pytest.importorskip("torch")


@pytest.fixture(scope="module")
def T(P):
    return P.display_thresholds()


def _device_display(P, torch, img, fmt, transfer, tone, exposure, pad=64):
    """the device's display of the (n, 3) host image, and the bytes behind it that it must leave alone"""
    from path_tracer_ocaml_amd import abi
    n = img.shape[0]
    b = P.display_pixel_bytes(fmt)
    d_rgb = torch.from_numpy(np.ascontiguousarray(img)).to("cuda:0")
    d_out = torch.full((n * b + pad,), 0xA5, dtype=torch.uint8, device="cuda:0")
    P.display_image_device(0, n, d_rgb.data_ptr(), d_out.data_ptr(), format=fmt, transfer=transfer, tone=tone, exposure=exposure)
    raw = d_out.cpu().numpy()
    assert np.all(raw[n * b:] == 0xA5), (fmt, n, "wrote beyond its pixels")
    dtype, ch = abi.PTX_PIXEL_LAYOUT[abi.PTX_PIXEL_NAMES.index(fmt)]
    return raw[:n * b].view(dtype).reshape(n, ch)


@pytest.mark.parametrize("fmt", R.FORMATS)
def test_device_equals_host_on_edge_values_at_every_setting_and_size(P, torch, T, fmt):
    images = {n: R.edge_image(T, n, seed=n) for n in SIZES}
    images["all"] = R.full_edge_image(T)  # every edge value, several workgroups
    for f, transfer, tone, exposure in R.settings():
        if f != fmt:
            continue
        for n, img in images.items():
            got = _device_display(P, torch, img, fmt, transfer, tone, exposure)
            want = P.display_apply(img, format=fmt, transfer=transfer, tone=tone, exposure=exposure)
            assert R.same(got, want), (fmt, transfer, tone, exposure, n, np.argwhere(got != want)[:4])
            assert R.same(want, R.apply(img, T, fmt, transfer, tone, exposure))


@pytest.mark.parametrize("fmt", R.FORMATS)
def test_a_range_writes_its_own_pixels_and_no_byte_beside_them(P, torch, T, fmt):
    """the ranges the row slabs of a pinned render take: starts and ends at every alignment to the kernel's four-pixel quads, ranges
    inside one quad, ranges over several workgroups.  Two adjacent ranges together write every byte once: the bytes outside a range
    keep the fill, so neither wrote into the other's quad."""
    from path_tracer_ocaml_amd import abi
    n = 1100  # 275 quads: two workgroups
    img = R.edge_image(T, n, seed=5)
    b = P.display_pixel_bytes(fmt)
    transfer, tone = ("srgb", "aces") if fmt.endswith("8") else ("linear", "reinhard")
    want = P.display_apply(img, format=fmt, transfer=transfer, tone=tone, exposure=0.5).view(np.uint8).reshape(n, b)
    d_rgb = torch.from_numpy(img).to("cuda:0")
    ranges = [(p0, p1) for p0 in (1, 2, 3, 4, 5, 6, 7, 1021, 1026) for p1 in (p0 + 1, p0 + 2, p0 + 3, p0 + 4, p0 + 5, 67, 134, 1099, 1100)
              if p0 < p1 <= n]
    for p0, p1 in ranges:
        d_out = torch.full((n * b,), 0xA5, dtype=torch.uint8, device="cuda:0")
        P.display_image_device(0, p1 - p0, d_rgb.data_ptr(), d_out.data_ptr(), format=fmt, transfer=transfer, tone=tone, exposure=0.5,
                               pixel_first=p0)
        got = d_out.cpu().numpy().reshape(n, b)
        assert np.all(got[:p0] == 0xA5) and np.all(got[p1:] == 0xA5), (fmt, p0, p1, "wrote outside its range")
        if fmt.endswith("32f"):  # (a NaN is a NaN: display_reference.same)
            dtype, ch = abi.PTX_PIXEL_LAYOUT[abi.PTX_PIXEL_NAMES.index(fmt)]
            assert R.same(got[p0:p1].copy().view(dtype), want[p0:p1].copy().view(dtype)), (fmt, p0, p1)
        else:
            assert np.array_equal(got[p0:p1], want[p0:p1]), (fmt, p0, p1)


def test_binary32_subnormal_results_are_numpys(P, torch, T):
    """what v_cvt_f32_f64 does under the kernel's denormal mode, measured: results inside the binary32 subnormal range, the ties
    between two subnormals and the values that round up into the normal range are numpy's astype(float32)"""
    sub = np.float64(2.0 ** -149)
    ks = np.arange(0, 64, dtype=np.float64)
    vals = np.concatenate([ks * sub, (ks + 0.5) * sub, np.nextafter((ks + 0.5) * sub, np.inf), np.nextafter((ks + 0.5) * sub, -np.inf),
                           2.0 ** -126 - ks * sub * 0.5, 2.0 ** -127 + ks * sub * 0.25])
    vals = np.concatenate([vals, -vals])
    img = np.resize(vals, (-(-len(vals) // 3), 3))
    got = _device_display(P, torch, img, "rgb32f", "reference", "none", 1.0)
    want = img.astype(np.float32)
    assert np.any((want != 0) & (np.abs(want) < np.finfo(np.float32).tiny))
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))


@pytest.fixture(scope="module")
def scenes(P, oracle):
    made = {}

    def get(kind, w, h):
        if (kind, w, h) not in made:
            d = (oracle.desc_shirley if kind == "shirley" else oracle.desc_cornell)(w, h)
            made[(kind, w, h)] = P.Scene(d.ptr, 0, keepalive=d)
        return made[(kind, w, h)]

    yield get
    for g in made.values():
        g.close()


SOME = (("rgb8", "reference", "none", 1.0), ("rgba8", "srgb", "aces", 0.25), ("rgb32f", "linear", "none", 1.0),
        ("rgba32f", "linear", "reinhard", 4.0), ("rgb8", "srgb", "none", 1.0), ("rgba8", "linear", "aces", 2.0))


@pytest.mark.parametrize("w, h", [(1, 1), (1, 257), (257, 1), (13, 11), (33, 9)])
def test_render_display_is_the_display_of_renders_image(P, scenes, w, h):
    g = scenes("shirley", w, h)
    for film in (None, (7, 3, True)):
        g.set_film(*(film or (5, 1, False)))
        rgb, st0 = g.render(w, h, SPP, DEPTH)
        for fmt, transfer, tone, exposure in SOME:
            got, st = g.render_display(w, h, SPP, DEPTH, format=fmt, transfer=transfer, tone=tone, exposure=exposure)
            want = P.display_apply(rgb, format=fmt, transfer=transfer, tone=tone, exposure=exposure)
            assert got.shape == want.shape and R.same(got, want), (w, h, film, fmt, transfer, tone)
            assert st["samples"] == st0["samples"] == w * h * SPP
    g.set_film(5, 1, False)


def test_render_display_of_a_lamp_lit_cornell_box(P, scenes):
    w, h = 40, 30
    g = scenes("cornell", w, h)
    rgb, _ = g.render(w, h, 4, DEPTH)
    assert rgb.max() > 1.0  # the emitter saturates the reference's conversion
    for fmt, transfer, tone, exposure in SOME:
        got, _ = g.render_display(w, h, 4, DEPTH, format=fmt, transfer=transfer, tone=tone, exposure=exposure)
        assert R.same(got, P.display_apply(rgb, format=fmt, transfer=transfer, tone=tone, exposure=exposure)), (fmt, transfer, tone)


@pytest.mark.parametrize("slabs", [1, 2, 3, 8])
def test_pinned_and_unpinned_at_an_odd_width_and_ragged_slabs(P, scenes, slabs, monkeypatch):
    """67 x 70: a slab starts at row0 * 67 pixels, no multiple of four, so neighbouring slabs share a quad of the display kernel"""
    from path_tracer_ocaml_amd import abi
    monkeypatch.setenv("PTX_FINAL_SLABS", str(slabs))
    w, h, spp = 67, 70, 4
    g = scenes("shirley", w, h)
    rgb, _ = g.render(w, h, spp, DEPTH, passes_per_batch=2)
    for fmt in R.FORMATS:
        transfer, tone, exposure = ("srgb", "aces", 0.5) if fmt.endswith("8") else ("linear", "reinhard", 0.5)
        want = P.display_apply(rgb, format=fmt, transfer=transfer, tone=tone, exposure=exposure)
        dtype, ch = abi.PTX_PIXEL_LAYOUT[abi.PTX_PIXEL_NAMES.index(fmt)]
        for ppb in (0, 2):  # (one pass per batch leaves no last batch to cut into slabs: the plain tail)
            plain, _ = g.render_display(w, h, spp, DEPTH, format=fmt, transfer=transfer, tone=tone, exposure=exposure, passes_per_batch=ppb)
            assert R.same(plain, want), (fmt, slabs, ppb, "unpinned")
            # the pinned image sits inside a larger registration: what lies around it must survive
            whole = np.full((h + 2, w, ch), 77, dtype=dtype)
            g.image_pin_bytes(whole)
            try:
                out = whole[1:h + 1]
                got, _ = g.render_display(w, h, spp, DEPTH, format=fmt, transfer=transfer, tone=tone, exposure=exposure, out=out,
                                          passes_per_batch=ppb)
            finally:
                g.unpin_image()
            assert R.same(got, want), (fmt, slabs, ppb, "pinned", np.argwhere(got != want)[:4])
            assert np.all(whole[0] == 77) and np.all(whole[h + 1] == 77)
    # the f64 pin still works through the byte-typed registration, and either kind is released by unpin
    img = np.full((h, w, 3), -1.0)
    g.pin_image(img)
    got, _ = g.render(w, h, spp, DEPTH, out=img, passes_per_batch=2)
    g.unpin_image()
    assert np.array_equal(got.view(np.uint64), rgb.view(np.uint64))


def test_two_aliased_replicas(P, scenes, monkeypatch):
    monkeypatch.setenv("PTX_MULTI_ALIAS", "1")  # test hook: replicas may share a device
    w, h = 33, 41
    g = scenes("shirley", w, h)
    rgb, _ = g.render(w, h, SPP, DEPTH)
    for fmt, transfer, tone, exposure in SOME[:4]:
        got, _ = g.render_display(w, h, SPP, DEPTH, format=fmt, transfer=transfer, tone=tone, exposure=exposure, n_gpus=2, band_rows=4)
        assert R.same(got, P.display_apply(rgb, format=fmt, transfer=transfer, tone=tone, exposure=exposure)), (fmt, transfer, tone)


@pytest.mark.parametrize("denoise", [False, True])
def test_progressive_display_updates_are_the_displays_of_the_f64_updates(P, scenes, denoise):
    w, h, n, k = 35, 27, 7, 3  # K ragged against N: updates after 3, 6 and 7 passes
    g = scenes("shirley", w, h)
    f64 = {}
    if denoise:
        g.render_denoised(w, h, n, DEPTH, k, on_update=lambda done, rel, rgb, err: f64.__setitem__(done, (rgb.copy(), err.copy(), rel)) and None)
    else:
        g.render_progressive(w, h, n, DEPTH, k, on_update=lambda done, rel, rgb, err: f64.__setitem__(done, (rgb.copy(), err.copy(), rel)) and None)
    assert sorted(f64) == [3, 6, 7]
    for fmt, transfer, tone, exposure in SOME[:3]:
        seen = {}

        def on_update(done, rel, pixels, err):
            seen[done] = (pixels.copy(), err.copy(), rel)

        out, err, done, st = g.render_progressive_display(w, h, n, DEPTH, k, denoise=denoise, format=fmt, transfer=transfer, tone=tone,
                                                          exposure=exposure, on_update=on_update)
        assert done == n and sorted(seen) == [3, 6, 7] and st["samples"] == w * h * n
        for j, (rgb_j, err_j, rel_j) in f64.items():
            want = P.display_apply(rgb_j, format=fmt, transfer=transfer, tone=tone, exposure=exposure)
            assert R.same(seen[j][0], want), (denoise, fmt, j)
            assert np.array_equal(seen[j][1].view(np.uint64), err_j.view(np.uint64)) and seen[j][2] == rel_j  # the error stays f64
        assert R.same(out, seen[n][0])
    if not denoise:  # run to N passes with REFERENCE / RGB8, out is the display of ptx_render's image
        rgb, _ = g.render(w, h, n, DEPTH)
        out, _, _, _ = g.render_progressive_display(w, h, n, DEPTH, k, want_error=False)
        assert np.array_equal(out, P.display_apply(rgb))
        # an early stop from the callback: the image of the update it stopped at
        out, _, done, st = g.render_progressive_display(w, h, n, DEPTH, k, transfer="srgb", on_update=lambda d, *a: d >= 3)
        assert done == 3 and st["samples"] == w * h * 3
        assert np.array_equal(out, P.display_apply(f64[3][0], transfer="srgb"))


def test_a_refused_call_leaves_out_untouched_and_the_handle_usable(P, scenes):
    from path_tracer_ocaml_amd import abi
    w, h = 13, 11
    g = scenes("shirley", w, h)
    L = P.lib()
    p = P.render_params(w, h, SPP, DEPTH)
    out = np.full((h, w, 4), 0xA5, dtype=np.uint8)
    bad = [abi.display_params(None, "rgb8", "reference", "aces", 1.0), abi.display_params(None, "rgb32f", "srgb", "none", 1.0),
           abi.display_params(None, 7, "linear", "none", 1.0), abi.display_params(None, "rgb8", "linear", "none", float("nan"))]
    pp = abi.ProgressiveParams()
    pp.passes_per_update = 2
    for d in bad:
        assert L.ptx_render_display(g._h, C.byref(p), C.byref(d), C.c_void_p(out.ctypes.data), None, None, None) == -1
        assert P.last_error().startswith("display: ")
        assert L.ptx_render_progressive_display(g._h, C.byref(p), C.byref(pp), None, C.byref(d), C.c_void_p(out.ctypes.data), None, None,
                                                None, None, None) == -1
        assert np.all(out == 0xA5)
    # good display settings, refused render parameters: still nothing written
    ok = P.display_defaults()
    p_bad = P.render_params(w, h, 0, DEPTH)
    assert L.ptx_render_display(g._h, C.byref(p_bad), C.byref(ok), C.c_void_p(out.ctypes.data), None, None, None) != 0
    assert L.ptx_render_display(g._h, C.byref(p), C.byref(ok), None, None, None, None) == -1
    assert np.all(out == 0xA5)
    rgb, _ = g.render(w, h, SPP, DEPTH)
    got, _ = g.render_display(w, h, SPP, DEPTH)
    assert np.array_equal(got, P.display_apply(rgb))


def test_the_display_kernel_is_not_in_the_launched_kernel_record(P, scenes):
    w, h = 33, 9
    g = scenes("shirley", w, h)
    assert not any("display" in name for name in P.kernel_table())
    g.clear_launched_kernels()
    g.render(w, h, SPP, DEPTH)
    plain = list(g.launched_kernels())
    g.clear_launched_kernels()
    g.render_display(w, h, SPP, DEPTH, format="rgba8", transfer="srgb", tone="aces", exposure=0.5)
    assert list(g.launched_kernels()) == plain and plain
