"""The film at any order and radius on the GPU: ptx_film_resolve_ex_device / _banded_ex_device / _counts_ex_device against the
restatement of the rule (tests/film_reference.py) bit for bit on seeded sums over twelve decades; the default film's identity with
the existing kernels; and every entry point that films through a scene -- ptx_render (a pinned image's row slabs included),
progressive, adaptive, denoised, multi -- against _ex_device of that scene's own raw sums."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import film_reference as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
IMAGES = [(1, 1), (1, 9), (9, 1), (3, 2), (33, 9), (65, 17), (40, 23)]  # (W, H); the last three straddle the 32 x 8 tile's edges
FILMS = [(1, 0), (5, 0), (3, 1), (5, 1), (7, 3), (16, 2), (15, 7), (16, 7)]


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


@pytest.fixture(scope="module")
def P():
    import path_tracer_ocaml_amd as P
    assert P.lib().ptx_device_count() >= 1, P.last_error()
    return P


@pytest.fixture(scope="module")
def torch():
    return pytest.importorskip("torch")


def _dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


def _zeros(torch, H, W):
    return torch.zeros((H, W, 3), dtype=torch.float64, device="cuda:0")


def _sums(W, H):
    return R.decades((H, W, 3), seed=100 * W + H)


def _ex(P, torch, S, film, spp):
    H, W, _ = S.shape
    d_raw, d_out = _dev(torch, S), _zeros(torch, H, W)
    P.film_resolve_device(0, W, H, spp, d_raw.data_ptr(), d_out.data_ptr(), film=film)
    return d_out.cpu().numpy()


def _same_bits(got, want, where):
    diff = bits(got) != bits(want)
    assert not diff.any(), (where, int(diff.sum()), np.argwhere(diff)[:3].tolist())


@pytest.mark.parametrize("order,radius", FILMS)
@pytest.mark.parametrize("W,H", IMAGES)
def test_ex_device_equals_the_restatement(P, torch, W, H, order, radius):
    S = _sums(W, H)
    acc, ws, clipped, _ = R.accumulate(S, order, radius)  # the taps once; the flags and spp only touch the last steps
    d_raw, d_out = _dev(torch, S), _zeros(torch, H, W)
    for flags in (0, 1):
        for spp in (1, 3, 64):
            d_out.fill_(-1.0)
            P.film_resolve_device(0, W, H, spp, d_raw.data_ptr(), d_out.data_ptr(), film=(order, radius, flags))
            got = d_out.cpu().numpy()
            assert np.isfinite(got).all()
            _same_bits(got, R.finish(acc, ws, clipped, flags, spp=spp), (W, H, order, radius, flags, spp))
    if radius > 0 and W * H > 1:
        assert clipped.any()
        a = R.finish(acc, ws, clipped, 0, spp=3)
        b = R.finish(acc, ws, clipped, 1, spp=3)
        assert (b[clipped] >= a[clipped]).all() and (b[clipped] > a[clipped]).any()  # the border no longer darkens


@pytest.mark.parametrize("W,H", [(65, 17), (600, 300)])
def test_the_default_film_through_ex_device_is_the_existing_film(P, torch, W, H, monkeypatch):
    S = R.decades((H, W, 3), seed=5)
    d_raw, a, b, c = _dev(torch, S), _zeros(torch, H, W), _zeros(torch, H, W), _zeros(torch, H, W)
    for spp in (1, 64):
        P.film_resolve_device(0, W, H, spp, d_raw.data_ptr(), a.data_ptr())
        P.film_resolve_device(0, W, H, spp, d_raw.data_ptr(), b.data_ptr(), film=(5, 1, False))
        P.film_resolve_device(0, W, H, spp, d_raw.data_ptr(), c.data_ptr(), film=None)
        assert torch.equal(a.view(torch.int64), b.view(torch.int64))
        assert torch.equal(a.view(torch.int64), c.view(torch.int64))
    # NULL film = the defaults
    c.fill_(-1.0)
    assert P.lib().ptx_film_resolve_ex_device(0, W, H, 64, None, d_raw.data_ptr(), c.data_ptr(), None) == 0
    assert torch.equal(a.view(torch.int64), c.view(torch.int64))
    # the counts pair on a mixed map
    rng = np.random.default_rng(9)
    counts = rng.integers(1, 9, (H, W)).astype(np.int32)
    counts[: H // 2, : W // 2] = 6
    d_n = _dev(torch, counts)
    P.film_resolve_counts_device(0, W, H, d_raw.data_ptr(), d_n.data_ptr(), a.data_ptr())
    P.film_resolve_counts_device(0, W, H, d_raw.data_ptr(), d_n.data_ptr(), b.data_ptr(), film=(5, 1))
    assert torch.equal(a.view(torch.int64), b.view(torch.int64))
    # PTX_FILM_WIDE=1 (the measurement switch of tools/film_cost.py) sends the default film through k_film_wide: the same bits
    monkeypatch.setenv("PTX_FILM_WIDE", "1")
    P.film_resolve_counts_device(0, W, H, d_raw.data_ptr(), d_n.data_ptr(), c.data_ptr())
    assert torch.equal(a.view(torch.int64), c.view(torch.int64))
    P.film_resolve_device(0, W, H, 64, d_raw.data_ptr(), c.data_ptr())
    monkeypatch.delenv("PTX_FILM_WIDE")
    P.film_resolve_device(0, W, H, 64, d_raw.data_ptr(), a.data_ptr())
    assert torch.equal(a.view(torch.int64), c.view(torch.int64))


@pytest.mark.parametrize("band_rows", [1, 3, 8])
@pytest.mark.parametrize("n_ranks", [1, 2, 3])
def test_banded_ex_reads_the_gathered_layout_in_place(P, torch, n_ranks, band_rows):
    """band_rows 1 and 3 are below the radius 7; the pad rows hold NaN: one in the output means a pad row was read"""
    W, H, spp = 40, 23, 3
    S = _sums(W, H)
    g, pad = R.to_banded(S, n_ranks, band_rows)
    assert np.isnan(g).any()
    d_g, d_out = _dev(torch, g), _zeros(torch, H, W)
    for film in ((15, 7, False), (15, 7, True), (7, 3, False), (5, 1, True), (5, 0, False)):
        d_out.fill_(-1.0)
        P.film_resolve_banded_device(0, W, H, spp, d_g.data_ptr(), n_ranks, band_rows, pad, d_out.data_ptr(), film=film)
        got = d_out.cpu().numpy()
        assert not np.isnan(got).any(), film
        _same_bits(got, _ex(P, torch, S, film, spp), (n_ranks, band_rows, film))
    with pytest.raises(P.PtxError, match="pad_rows"):
        P.film_resolve_banded_device(0, W, H, spp, d_g.data_ptr(), n_ranks, band_rows, 0, d_out.data_ptr(), film=(7, 3))


def _counts_ex(P, torch, S, counts, film):
    H, W, _ = S.shape
    d_raw, d_n, d_out = _dev(torch, S), _dev(torch, counts.astype(np.int32)), _zeros(torch, H, W)
    P.film_resolve_counts_device(0, W, H, d_raw.data_ptr(), d_n.data_ptr(), d_out.data_ptr(), film=film)
    return d_out.cpu().numpy()


@pytest.mark.parametrize("film", [(5, 0, 0), (7, 3, 0), (7, 3, 1), (15, 7, 1)])
def test_counts_ex_with_a_uniform_map_is_ex_device_with_spp_n(P, torch, film):
    W, H, n = 40, 23, 6
    S = _sums(W, H)
    got = _counts_ex(P, torch, S, np.full((H, W), n), film)
    _same_bits(got, _ex(P, torch, S, film, n), film)


@pytest.mark.parametrize("W,H,film", [(33, 9, (7, 3, 0)), (33, 9, (7, 3, 1)), (40, 23, (3, 1, 1)), (9, 1, (15, 7, 0)), (33, 9, (5, 0, 0))])
def test_counts_ex_with_a_mixed_map_equals_the_restatement(P, torch, W, H, film):
    S = _sums(W, H)
    rng = np.random.default_rng(W + H)
    counts = rng.integers(1, 9, (H, W)).astype(np.int32)
    counts[:, : W // 2] = 5  # a region where whole windows agree
    got = _counts_ex(P, torch, S, counts, film)
    assert np.isfinite(got).all()
    _same_bits(got, R.film_counts(S, counts, *film), (W, H, film))


def test_counts_ex_sees_a_foreign_count_at_the_edge_of_its_own_window(P, torch):
    """the only foreign count sits at distance 3 from the pixel: a 3 x 3 window would call the pixel `same`, the 7 x 7 one must not"""
    W, H, film = 16, 12, (7, 3, 0)
    S = _sums(W, H) + 1.0
    counts = np.full((H, W), 4, dtype=np.int32)
    counts[6, 8] = 9
    want = R.film_counts(S, counts, *film)
    _, _, _, same = R.accumulate(S, 7, 3, counts)
    assert not same[6, 5] and not same[3, 8] and not same[9, 11] and same[6, 4] and same[2, 8]
    got = _counts_ex(P, torch, S, counts, film)
    _same_bits(got, want, "distance 3")
    uniform = _ex(P, torch, S, film, 4)
    assert (bits(got[6, 5]) != bits(uniform[6, 5])).any()   # ... and the pixel's value shows it
    _same_bits(got[6, 4], uniform[6, 4], "distance 4")
    near = _counts_ex(P, torch, S, counts, (5, 1, 0))         # the 3 x 3 window does call it `same`
    _same_bits(near[6, 5], _ex(P, torch, S, (5, 1, 0), 4)[6, 5], "3 x 3 window")


# ---- through a scene

SHIRLEY = (48, 24, 4, 3)  # W, H, spp, depth


@pytest.fixture(scope="module")
def shirley(P, torch, oracle):
    """(scene with film (7, 3), _ex_device (7, 3) of its own raw sums, the raw sums on the device)"""
    w, h, spp, depth = SHIRLEY
    d = oracle.desc_shirley(w, h)
    g = P.Scene(d.ptr, 0, keepalive=d)
    raw = _zeros(torch, h, w)
    g.render_raw_device(P.render_params(w, h, spp, depth), raw.data_ptr())
    out = _zeros(torch, h, w)
    P.film_resolve_device(0, w, h, spp, raw.data_ptr(), out.data_ptr(), film=(7, 3))
    g.set_film(7, 3)
    yield g, out.cpu().numpy(), raw
    g.close()


def test_render_films_with_the_scenes_film(P, torch, shirley):
    g, want, raw = shirley
    w, h, spp, depth = SHIRLEY
    assert g.film() == (7, 3, False)
    got, _ = g.render(w, h, spp, depth)
    _same_bits(got, want, "ptx_render")
    plain = _zeros(torch, h, w)
    P.film_resolve_device(0, w, h, spp, raw.data_ptr(), plain.data_ptr())
    assert (bits(plain.cpu().numpy()) != bits(want)).any()  # the film does change the image


def test_progressive_run_to_n_films_with_the_scenes_film(shirley):
    g, want, _ = shirley
    w, h, spp, depth = SHIRLEY
    got, _, done, _ = g.render_progressive(w, h, spp, depth, 3)
    assert done == spp
    _same_bits(got, want, "ptx_render_progressive")


def test_denoised_at_zero_levels_films_with_the_scenes_film(shirley):
    g, want, _ = shirley
    w, h, spp, depth = SHIRLEY
    got, _, _, done, _ = g.render_denoised(w, h, spp, depth, 2, denoise={"levels": 0})
    assert done == spp
    _same_bits(got, want, "ptx_render_denoised")


def test_two_aliased_replicas_film_with_the_film_of_the_first(P, shirley, monkeypatch):
    g, want, _ = shirley
    w, h, spp, depth = SHIRLEY
    monkeypatch.setenv("PTX_MULTI_ALIAS", "1")
    r = g.replicate(0)
    assert r.film() == (7, 3, False)  # ptx_scene_replicate copies the film
    r.set_film(5, 0)                  # ... and the film of scenes[0] governs
    got, _ = P.render_multi([g, r], w, h, spp, depth, band_rows=2)  # bands below the radius
    _same_bits(got, want, "ptx_render_multi")
    got, _ = g.render(w, h, spp, depth, n_gpus=2, band_rows=2)
    _same_bits(got, want, "n_gpus = 2")
    r.close()


def test_adaptive_at_target_zero_films_with_the_scenes_film(P, torch, oracle):
    w, h, spp, depth = 24, 24, 4, 3
    d = oracle.desc_cornell(w, h)
    g = P.Scene(d.ptr, 0, keepalive=d)
    raw, out = _zeros(torch, h, w), _zeros(torch, h, w)
    g.render_raw_device(P.render_params(w, h, spp, depth), raw.data_ptr())
    P.film_resolve_device(0, w, h, spp, raw.data_ptr(), out.data_ptr(), film=(7, 3))
    g.set_film(7, 3)
    got, _, passes, _ = g.render_adaptive(w, h, spp, depth, 0.0, min_passes=2, passes_per_round=1)
    assert (passes == spp).all()
    _same_bits(got, out.cpu().numpy(), "ptx_render_adaptive")
    g.close()


def test_the_film_is_sticky_and_cannot_change_under_a_render(P, oracle):
    from path_tracer_ocaml_amd import abi
    w, h, spp, depth = SHIRLEY
    d = oracle.desc_shirley(w, h)
    fresh, g = P.Scene(d.ptr, 0, keepalive=d), P.Scene(d.ptr, 0, keepalive=d)
    ref, _ = fresh.render(w, h, spp, depth)
    g.set_film(15, 7, renormalise=True)
    wide, _ = g.render(w, h, spp, depth)
    assert (bits(wide) != bits(ref)).any()
    again, _ = g.render(w, h, spp, depth)
    _same_bits(again, wide, "sticky")
    rcs = []
    f = abi.FilmParams(5, 0, 0, 0)

    def progress(n):
        rcs.append(P.lib().ptx_scene_set_film(g._h, C.byref(f)))
        rcs.append(P.lib().ptx_scene_set_film(g._h, None))

    during, _ = g.render(w, h, spp, depth, progress=progress)
    assert rcs and set(rcs) == {-3}
    assert "film" in P.last_error()
    assert g.film() == (15, 7, True)
    _same_bits(during, wide, "the render finishes with the old film")
    assert P.lib().ptx_scene_set_film(g._h, None) == 0
    back, _ = g.render(w, h, spp, depth)
    _same_bits(back, ref, "NULL restores the default")
    fresh.close()
    g.close()


@pytest.mark.parametrize("slabs", [4, 8])
@pytest.mark.parametrize("h", [70, 64])
def test_a_pinned_images_row_slabs_read_the_radius_beyond(P, oracle, h, slabs, monkeypatch):
    """ptx_render into a pinned image films slab k once slab k + 1 has been summed; with radius 7 a slab's film reads 7 rows beyond it
    (8 slabs over 64 rows: 8-row slabs, the tightest case)"""
    monkeypatch.setenv("PTX_FINAL_SLABS", str(slabs))
    w, depth = 16, 3
    d = oracle.desc_shirley(w, h)
    g = P.Scene(d.ptr, 0, keepalive=d)
    img = np.full((h, w, 3), -1.0)
    for film in ((15, 7, False), (15, 7, True), (5, 0, False)):
        g.set_film(*film)
        for spp, ppb in ((4, 0), (4, 2)):
            ref, _ = g.render(w, h, spp, depth, passes_per_batch=ppb)  # unpinned: one film launch
            g.pin_image(img)
            img[:] = -1.0
            g.render(w, h, spp, depth, out=img, passes_per_batch=ppb)
            g.unpin_image()
            _same_bits(img, ref, (film, spp, ppb))
    g.close()


def _cli(*args):
    exe = os.path.join(ROOT, "path_tracer_ocaml_amd", "shirley_spheres")
    env = dict(os.environ)
    env["LD_LIBRARY_PATH"] = "/opt/rocm/lib:" + env.get("LD_LIBRARY_PATH", "")
    return subprocess.run([exe, "--no-progress", *args], capture_output=True, text=True, env=env, timeout=120)


def test_cli_filter_flags(P, tmp_path):
    from path_tracer_ocaml_amd import host as H
    w, h, spp, depth = 48, 24, 4, 3
    hs = H.shirley_spheres(w, h)
    g = P.Scene(hs.ptr, 0, keepalive=hs)
    g.set_film(7, 3, renormalise=True)
    rgb, _ = g.render(w, h, spp, depth)
    g.close()
    H.write_png(str(tmp_path / "py.png"), rgb)
    out = tmp_path / "cli.png"
    r = _cli(f"--dimension={w},{h}", f"--samples-per-pixel={spp}", f"--max-ray-bounces={depth}", "--filter=7,3", "--filter-renormalise",
             "-o", str(out))
    assert r.returncode == 0, r.stderr
    assert out.read_bytes() == (tmp_path / "py.png").read_bytes()
    bad = tmp_path / "bad.png"
    r = _cli(f"--dimension={w},{h}", "--filter=5,3", "-o", str(bad))
    assert r.returncode != 0 and "2 * pixel_radius + 1" in r.stderr and r.stdout == ""
    assert not bad.exists()
