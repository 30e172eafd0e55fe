"""`shirley_spheres` behind the display entry points, on the GPU.  With no display flag the PNG of the plain render, of --progressive and
of --denoise holds the bytes write_png makes of Python's f64 image (the files the CLI always wrote); with --transfer / --tone /
--exposure it holds display_apply of that image; --hdr-out is the RGB32F / linear display of the image whatever the flags say; the
drivers that keep their f64 image (--adaptive) convert it by the same rule; a refused combination exits 124 with the rule."""
import os
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H, SPP, DEPTH = 40, 24, 4, 2


@pytest.fixture(scope="module")
def P():
    import path_tracer_ocaml_amd as P
    assert P.lib().ptx_device_count() >= 1, P.last_error()
    return P


def _cli(tmp_path, name, *flags, ok=True):
    env = dict(os.environ)
    env["LD_LIBRARY_PATH"] = "/opt/rocm/lib:" + env.get("LD_LIBRARY_PATH", "")
    exe = os.path.join(ROOT, "path_tracer_ocaml_amd", "shirley_spheres")
    png = tmp_path / f"{name}.png"
    r = subprocess.run([exe, f"--dimension={W},{H}", f"--samples-per-pixel={SPP}", f"--max-ray-bounces={DEPTH}", "--no-progress",
                        "-o", str(png), *flags], capture_output=True, text=True, env=env, timeout=300)
    if ok:
        assert r.returncode == 0, r.stderr
    return png, r


def _png_of(tmp_path, name, pixels, f64):
    from path_tracer_ocaml_amd import host as Hs
    path = tmp_path / f"{name}.png"
    (Hs.write_png if f64 else Hs.write_png8)(str(path), pixels)
    return path.read_bytes()


@pytest.fixture(scope="module")
def shirley(P):
    from path_tracer_ocaml_amd import host as Hs
    hs = Hs.shirley_spheres(W, H)
    g = P.Scene(hs.ptr, 0, keepalive=hs)
    yield g
    g.close()


def test_with_no_display_flag_the_png_is_write_png_of_pythons_image(P, shirley, tmp_path):
    rgb, _ = shirley.render(W, H, SPP, DEPTH)
    want = _png_of(tmp_path, "py", rgb, True)
    assert _cli(tmp_path, "plain")[0].read_bytes() == want
    png, r = _cli(tmp_path, "prog", "--progressive=2")
    assert png.read_bytes() == want
    assert [l.split(",")[0] for l in r.stdout.splitlines() if l.startswith("#passes")] == ["#passes = 2", "#passes = 4"]
    den, _, _, _, _ = shirley.render_denoised(W, H, SPP, DEPTH, SPP)
    assert _cli(tmp_path, "den", "--denoise")[0].read_bytes() == _png_of(tmp_path, "py_den", den, True)
    # a driver that keeps its f64 image converts it by the same rule: T = 0 gives every pixel all passes, ptx_render's image
    assert _cli(tmp_path, "adaptive", "--adaptive=0", "--min-passes=2")[0].read_bytes() == want


def test_display_flags_on_the_lamp_lit_cornell_box(P, tmp_path):
    from path_tracer_ocaml_amd import host as Hs
    hs = Hs.cornell_lamp(W, H, 12.0, 0.03, 0.999, 400.0)
    g = P.Scene(hs.ptr, 0, keepalive=hs)
    rgb, _ = g.render(W, H, SPP, DEPTH)
    assert rgb.max() > 1.0  # the lamp saturates the reference's conversion
    scene = ("--scene=cornell", "--lamp=0.03,0.999,400")
    flags = ("--transfer=srgb", "--tone=aces", "--exposure=0.25")
    want = P.display_apply(rgb, transfer="srgb", tone="aces", exposure=0.25)
    want_png = _png_of(tmp_path, "py", want, False)
    assert _cli(tmp_path, "plain", *scene, *flags)[0].read_bytes() == want_png
    assert _cli(tmp_path, "prog", *scene, *flags, "--progressive=3")[0].read_bytes() == want_png
    assert _cli(tmp_path, "adaptive", *scene, *flags, "--adaptive=0", "--min-passes=2")[0].read_bytes() == want_png
    assert want_png != _png_of(tmp_path, "ref", rgb, True)
    # --hdr-out: the RGB32F / linear / no-tone display at exposure 1 of the same image, with and without the display flags
    for name, extra in (("hdr", ()), ("hdr_flags", flags)):
        pfm = tmp_path / f"{name}.pfm"
        png, _ = _cli(tmp_path, name, *scene, *extra, f"--hdr-out={pfm}")
        got = Hs.load_pfm(str(pfm))
        lin = P.display_apply(rgb, format="rgb32f", transfer="linear", tone="none", exposure=1.0)
        assert got.shape == (H, W, 3) and np.array_equal(got.astype(np.float32).view(np.uint32), lin.view(np.uint32))
        assert np.array_equal(lin, (rgb * rgb).astype(np.float32))  # the square it always wrote
        assert png.read_bytes() == (want_png if extra else _png_of(tmp_path, "ref2", rgb, True))
    g.close()


def test_refused_display_flags_exit_124_with_the_rule(tmp_path):
    for flags, message in ((("--tone=aces",), "PTX_TRANSFER_REFERENCE needs"), (("--exposure=2",), "PTX_TRANSFER_REFERENCE needs"),
                           (("--transfer=gamma",), "--transfer"), (("--tone=filmic", "--transfer=srgb"), "--tone"),
                           (("--exposure=-1", "--transfer=srgb"), "--exposure"), (("--exposure=nan", "--transfer=srgb"), "--exposure")):
        png, r = _cli(tmp_path, "bad", *flags, ok=False)
        assert r.returncode == 124 and message in r.stderr, (flags, r.returncode, r.stderr)
        assert not png.exists()
