"""The OCaml binding's display functions (Ptx.display_defaults / Ptx.render_display / Ptx.render_progressive_display): the calls the
stubs make, compiled and run from C against the real C ABI -- on a host-only scene here, and on the GPU in every format against
ptx_render + ptx_display_apply called with structs filled in by hand -- and the stubs type-checked against the runtime's documented C
interface (tests/c/mock_caml).  OCaml itself is not needed."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B = os.path.join(ROOT, "bindings", "ocaml")
LIBDIR = os.path.join(ROOT, "path_tracer_ocaml_amd")


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("ocaml_display") / "driver")
    subprocess.check_call(["gcc", "-O1", "-Wall", "-Werror", "-Wno-unused-function", "-I", os.path.join(ROOT, "include"), "-I", B,
                           os.path.join(ROOT, "tests", "c", "ocaml_display_driver.c"), "-o", exe, "-L", LIBDIR, "-lptx_hip", "-lm",
                           "-Wl,-rpath," + LIBDIR, "-Wl,-rpath-link,/opt/rocm/lib"])
    return exe


def _lines(exe, *args):
    out = subprocess.check_output([exe, *args], text=True)
    return {l.split()[0]: l.split(None, 2)[1:] for l in out.splitlines()}


def test_the_stub_calls_drive_the_c_abi(driver):
    lines = _lines(driver)
    assert lines["defaults"] == ["0", "0 0 0 1"]  # RGB8, REFERENCE, NONE, exposure 1
    assert [lines["channels%d" % f] for f in range(-1, 5)] == [["0", "0"], ["3", "0"], ["4", "0"], ["3", "1"], ["4", "1"], ["0", "0"]]
    assert lines["null_params"] == ["-1", "-1"]
    assert lines["host_only"][0] == "-3" and "host-only" in lines["host_only"][1]  # PTX_ERR_STATE, from the library
    assert lines["null_scene"][0] == "-1"
    for name, words in (("bad_format", "unknown format 9"), ("bad_transfer", "unknown transfer 7"), ("bad_tone", "unknown tone 5"),
                        ("bad_exposure", "exposure must be finite"), ("reference_tone", "PTX_TRANSFER_REFERENCE needs"),
                        ("f32_srgb", "binary32 formats"), ("u_bad_format", "unknown format 9"), ("u_bad_transfer", "unknown transfer 7"),
                        ("u_bad_tone", "unknown tone 5"), ("u_bad_exposure", "exposure must be finite")):
        assert lines[name][0] == "-1" and words in lines[name][1], (name, lines[name])  # every slot lands in its field
    assert lines["small"] == ["-4"] and lines["u_small"] == ["-4"]  # an image too small for the format never reaches the library
    assert lines["small_rgb8"] == ["-3"]  # ... and one that is large enough does
    assert lines["u_host_only"][0] == "-3"


@pytest.mark.gpu
def test_the_marshalled_frames_and_updates_are_the_c_abis(driver):
    lines = _lines(driver, "0")
    for f in range(4):
        assert lines["frame%d" % f] == ["0", "0 1 1 1 1"], (f, lines["frame%d" % f])  # same bytes, nothing beyond, sized, not black
    assert lines["updates0"] == ["0", "0 1 1 4 4"]
    assert lines["updates1"] == ["0", "0 1 1 4 4"]
    assert lines["bad_levels"][0] == "-1" and "levels" in lines["bad_levels"][1]
    assert lines["bad_sigma_a"][0] == "-1" and "sigma" in lines["bad_sigma_a"][1]
    assert lines["unread_denoiser"][0] == "0"  # without denoise the denoiser's slots are not read


def test_stubs_typecheck_and_agree_with_the_ml_file():
    subprocess.check_call(["gcc", "-std=gnu11", "-Wall", "-Wextra", "-Werror", "-fsyntax-only",
                           "-I", os.path.join(ROOT, "tests", "c", "mock_caml"), "-I", os.path.join(ROOT, "include"), "-I", B,
                           os.path.join(B, "ptx_stubs.c")])
    ml = open(os.path.join(B, "ptx.ml")).read()
    c = open(os.path.join(B, "ptx_stubs.c")).read()
    for stub, arity, externals in (("ptx_ml_display_defaults_stub", 1, 1), ("ptx_ml_render_display_stub", 4, 2),
                                   ("ptx_ml_render_progressive_display_stub", 5, 2)):
        m = re.search(r"CAMLprim value %s\(([^)]*)\)" % stub, c)
        assert m and len(m.group(1).split(",")) == arity
        exts = re.findall(r"external \w+\s*:([^=]*)= \"%s\"" % stub, ml, flags=re.S)
        assert len(exts) == externals, stub  # one external per element type of the display image
        for ext in exts:
            ext = re.sub(r"\(\*.*?\*\)", "", ext, flags=re.S)
            arrows = len(re.findall(r"^\s*->", ext, flags=re.M)) if "\n" in ext.strip() else ext.count("->")  # top-level arrows
            assert arrows == arity, stub
    for name in ("display_defaults", "render_display", "render_progressive_display", "create_pixels"):
        assert re.search(r"^let %s\b" % name, ml, flags=re.M), name
    assert "int8_unsigned_elt" in ml and "float32_elt" in ml
    # the wrappers hand over as many floats as the stubs ask for and the marshal functions read
    assert "floatarray_length(params) != 9" in c and "floatarray_length(params) != 18" in c
    body = ml[ml.index("let render_display "):ml.index("let render_progressive_display")]
    assert body.count("Float.of_int") == 5 and "@ display_floats display" in body
    flo = ml[ml.index("let display_floats"):ml.index("let create_pixels")]
    assert len(re.findall(r"^\s*[\[;] ", flo, flags=re.M)) == 4
    body = ml[ml.index("let render_progressive_display"):]
    assert len(re.findall(r"^\s*(?:\(|@ )?[\[;] ", body[body.index("FA.of_list"):body.index("let callback")], flags=re.M)) == 6 + 8
    assert "@ display_floats display" in body
    h = open(os.path.join(B, "ptx_ml_marshal.h")).read()
    assert "ptx_render_display(" in h and "ptx_render_progressive_display(" in h and "ptx_display_defaults(" in h
    assert "params9 + 5" in h and "params18 + 6" in h and "params18[17]" in h
    # the codes the ml file sends are the header's
    hdr = open(os.path.join(ROOT, "include", "ptx.h")).read()
    for define, code in (("PTX_PIXEL_RGB8", 0), ("PTX_PIXEL_RGBA8", 1), ("PTX_PIXEL_RGB32F", 2), ("PTX_PIXEL_RGBA32F", 3),
                         ("PTX_TRANSFER_REFERENCE", 0), ("PTX_TRANSFER_LINEAR", 1), ("PTX_TRANSFER_SRGB", 2), ("PTX_TONE_NONE", 0),
                         ("PTX_TONE_REINHARD", 1), ("PTX_TONE_ACES", 2)):
        assert re.search(r"#define %s %d\b" % (define, code), hdr), define
    for ctor, code in (("Rgb8", 0), ("Rgba8", 1), ("Rgb32f", 2), ("Rgba32f", 3), ("Reference", 0), ("Linear", 1), ("Srgb", 2),
                       ("No_tone", 0), ("Reinhard", 1), ("Aces", 2)):
        assert re.search(r"\| %s -> %d\b" % (ctor, code), ml), ctor
