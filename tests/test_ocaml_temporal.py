"""The OCaml binding's temporal functions (Ptx.render_temporal / Ptx.temporal_reset): the calls the stubs make, compiled and run from
C against the real C ABI -- on a host-only scene here, and on the GPU frame for frame against ptx_render_temporal called with structs
filled in by hand -- and the stubs type-checked against the runtime's documented C interface (tests/c/mock_caml).  OCaml itself is
not needed."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B = os.path.join(ROOT, "bindings", "ocaml")
LIBDIR = os.path.join(ROOT, "path_tracer_ocaml_amd")


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("ocaml_temporal") / "driver")
    subprocess.check_call(["gcc", "-O1", "-Wall", "-Werror", "-Wno-unused-function", "-I", os.path.join(ROOT, "include"), "-I", B,
                           os.path.join(ROOT, "tests", "c", "ocaml_temporal_driver.c"), "-o", exe, "-L", LIBDIR, "-lptx_hip", "-lm",
                           "-Wl,-rpath," + LIBDIR, "-Wl,-rpath-link,/opt/rocm/lib"])
    return exe


def _lines(exe, *args):
    out = subprocess.check_output([exe, *args], text=True)
    return {l.split()[0]: l.split(None, 2)[1:] for l in out.splitlines()}


def test_the_stub_calls_drive_the_c_abi(driver):
    lines = _lines(driver)
    assert lines["null_params"] == ["-1"]
    assert lines["host_only"][0] == "-3" and "host-only" in lines["host_only"][1]  # PTX_ERR_STATE, from the library
    assert lines["null_scene"][0] == "-1" and "NULL scene" in lines["null_scene"][1]
    assert lines["reset"] == ["0"]
    assert lines["reset_null"][0] == "-1" and "NULL scene" in lines["reset_null"][1]


@pytest.mark.gpu
def test_the_marshalled_frames_are_the_c_abis(driver):
    lines = _lines(driver, "0")
    for f in range(3):  # frame 2 with the spatial filter
        rc_a, rest = lines["frame%d" % f]
        rc_b, same, took_a, took_b, top = rest.split()
        assert (rc_a, rc_b, same) == ("0", "0", "1"), (f, lines["frame%d" % f])
        assert took_a == took_b and float.fromhex(top) > 0.0
        assert (int(took_a) == 0) == (f == 0), (f, took_a)  # a still camera: history from the second frame on
    for name, words in (("bad_width", "dimensions"), ("bad_height", "dimensions"), ("bad_spp", "samples_per_pixel"), ("bad_depth", "max_bounces"),
                        ("bad_first", "pass range"), ("bad_count", "pass_count"), ("bad_cap", "max_history_passes"),
                        ("bad_threshold", "normal_threshold"), ("bad_tolerance", "depth_tolerance"), ("bad_weight", "min_weight"),
                        ("bad_levels", "levels"), ("bad_power", "normal_power_log2"), ("bad_passes", "feature_passes"), ("bad_flags", "flags"),
                        ("bad_sigma_l", "sigma"), ("bad_sigma_z", "sigma"), ("bad_sigma_a", "sigma")):
        assert lines[name][0] == "-1" and words in lines[name][1], (name, lines[name])  # every slot lands in its field
    assert lines["unread_denoiser"][0] == "0"
    assert lines["reset"] == ["0"] and lines["after_reset"] == ["0", "0"]


def test_stubs_typecheck_and_agree_with_the_ml_file():
    subprocess.check_call(["gcc", "-std=gnu11", "-Wall", "-Wextra", "-Werror", "-fsyntax-only",
                           "-I", os.path.join(ROOT, "tests", "c", "mock_caml"), "-I", os.path.join(ROOT, "include"), "-I", B,
                           os.path.join(B, "ptx_stubs.c")])
    ml = open(os.path.join(B, "ptx.ml")).read()
    c = open(os.path.join(B, "ptx_stubs.c")).read()
    for stub, arity in (("ptx_ml_render_temporal_stub", 5), ("ptx_ml_temporal_reset_stub", 1)):
        assert '"%s"' % stub in ml
        m = re.search(r"CAMLprim value %s\(([^)]*)\)" % stub, c)
        assert m and len(m.group(1).split(",")) == arity
        ext = re.search(r"external \w+\s*: ([^=]*)= \"%s\"" % stub, ml, flags=re.S)
        assert ext and re.sub(r"\(\*.*?\*\)", "", ext.group(1), flags=re.S).count("->") == arity
    assert re.search(r"^let render_temporal\b", ml, flags=re.M) and re.search(r"^external temporal_reset\b", ml, flags=re.M)
    # the wrapper hands over as many floats as the stub asks for and the marshal function reads
    body = ml[ml.index("let render_temporal"):ml.index("render_temporal_flat scene params")]
    assert len(re.findall(r"^\s*[\[;] ", body[body.index("FA.of_list"):], flags=re.M)) == 18
    assert "floatarray_length(params) != 18" in c and "ptx_ml_render_temporal(" in c and "ptx_ml_temporal_reset(" in c
    h = open(os.path.join(B, "ptx_ml_marshal.h")).read()
    assert "ptx_render_temporal(" in h and "ptx_temporal_reset(" in h and "params18[17]" in h
