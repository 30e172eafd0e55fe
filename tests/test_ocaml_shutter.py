"""The OCaml binding's camera-shutter functions (Ptx.set_camera_shutter / Ptx.clear_camera_shutter / Ptx.camera_shutter): the calls the
stubs make, compiled and run from C against the real C ABI on a host-only scene, and the stubs type-checked against the runtime's
documented C interface (tests/c/mock_caml).  OCaml itself is not needed."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B = os.path.join(ROOT, "bindings", "ocaml")
LIBDIR = os.path.join(ROOT, "path_tracer_ocaml_amd")
MOTION = [0.25, -1.5, float.fromhex("0x1.23456789abcdep+3"), 0.6, 0.0, -0.8, -0.75]


@pytest.fixture(scope="module")
def lines(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("ocaml_shutter") / "driver")
    subprocess.check_call(["gcc", "-O1", "-Wall", "-Werror", "-Wno-unused-function", "-I", os.path.join(ROOT, "include"), "-I", B,
                           os.path.join(ROOT, "tests", "c", "ocaml_shutter_driver.c"), "-o", exe, "-L", LIBDIR, "-lptx_hip",
                           "-Wl,-rpath," + LIBDIR, "-Wl,-rpath-link,/opt/rocm/lib"])
    out = subprocess.check_output([exe], text=True)
    return {l.split()[0]: l.split(None, 2)[1:] for l in out.splitlines()}


def _state(rest):
    """(on, the 7 doubles)"""
    words = rest.split()
    return int(words[0]), [float.fromhex(v) for v in words[1:]]


def test_the_stub_calls_drive_the_c_abi(lines):
    assert lines["initial"][0] == "0" and _state(lines["initial"][1]) == (0, [0.0] * 7)
    assert lines["set"][0] == "0" and _state(lines["set"][1]) == (1, MOTION)  # the doubles arrive bit for bit
    for name, words in (("nan_translation", "translation must be finite"), ("not_unit", "| |axis| - 1 |"), ("wide_angle", "|angle| must be at most pi")):
        assert lines[name][0] == "-1" and lines[name][1].startswith("camera shutter: ") and words in lines[name][1], name
    assert lines["kept"] == lines["set"]  # a refused call changes nothing
    assert lines["still"][0] == "0" and _state(lines["still"][1]) == (1, [0.0] * 7)  # no motion is still a shutter: ON
    assert lines["clear"][0] == "0" and _state(lines["clear"][1]) == (0, [0.0] * 7)
    assert lines["null"][0] == "-1" and "NULL scene" in lines["null"][1]
    # the lengths are checked before anything is read
    assert lines["short_motion"] == ["-4"] and lines["long_motion"] == ["-4"] and lines["short_out"] == ["-4"]
    assert lines["still_clear"] == lines["clear"]


def test_stubs_typecheck_and_agree_with_the_ml_file():
    subprocess.check_call(["gcc", "-std=gnu11", "-Wall", "-Wextra", "-Werror", "-fsyntax-only",
                           "-I", os.path.join(ROOT, "tests", "c", "mock_caml"), "-I", os.path.join(ROOT, "include"), "-I", B,
                           os.path.join(B, "ptx_stubs.c")])
    ml = open(os.path.join(B, "ptx.ml")).read()
    c = open(os.path.join(B, "ptx_stubs.c")).read()
    for stub, arity in (("ptx_ml_set_camera_shutter_stub", 2), ("ptx_ml_clear_camera_shutter_stub", 1), ("ptx_ml_camera_shutter_stub", 2)):
        assert '"%s"' % stub in ml
        m = re.search(r"CAMLprim value %s\(([^)]*)\)" % stub, c)
        assert m and len(m.group(1).split(",")) == arity
        ext = re.search(r"external \w+\s*: ([^=]*)= \"%s\"" % stub, ml)
        assert ext and ext.group(1).count("->") == arity
    for name in ("set_camera_shutter", "camera_shutter"):
        assert re.search(r"^let %s\b" % name, ml, flags=re.M)
    assert re.search(r"^external clear_camera_shutter\b", ml, flags=re.M)
    assert "ptx_ml_set_camera_shutter(" in c and "ptx_ml_clear_camera_shutter(" in c and "ptx_ml_camera_shutter(" in c
    h = open(os.path.join(B, "ptx_ml_marshal.h")).read()
    assert "ptx_scene_set_camera_shutter(" in h and "ptx_scene_camera_shutter(" in h
