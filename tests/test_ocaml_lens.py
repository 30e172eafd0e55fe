"""The OCaml binding's thin-lens functions (Ptx.set_lens / Ptx.lens): the calls the stubs make, compiled and run from C against the
real C ABI on a host-only scene, and the stubs type-checked against the runtime's documented C interface (tests/c/mock_caml).  OCaml
itself is not needed."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B = os.path.join(ROOT, "bindings", "ocaml")
LIBDIR = os.path.join(ROOT, "path_tracer_ocaml_amd")


@pytest.fixture(scope="module")
def lines(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("ocaml_lens") / "driver")
    subprocess.check_call(["gcc", "-O1", "-Wall", "-Werror", "-Wno-unused-function", "-I", os.path.join(ROOT, "include"), "-I", B,
                           os.path.join(ROOT, "tests", "c", "ocaml_lens_driver.c"), "-o", exe, "-L", LIBDIR, "-lptx_hip",
                           "-Wl,-rpath," + LIBDIR, "-Wl,-rpath-link,/opt/rocm/lib"])
    out = subprocess.check_output([exe], text=True)
    return {l.split()[0]: l.split(None, 2)[1:] for l in out.splitlines()}


def _pair(rest):
    return tuple(float.fromhex(v) for v in rest.split())


def test_the_stub_calls_drive_the_c_abi(lines):
    assert lines["initial"][0] == "0" and _pair(lines["initial"][1]) == (0.0, 1.0)
    assert lines["set"][0] == "0" and _pair(lines["set"][1]) == (0.05, 13.5)  # the doubles arrive bit for bit
    for name, words in (("negative", "radius must be finite and >= 0"), ("nan", "radius must be finite and >= 0"),
                        ("no_focus", "focus_distance must be finite and > 0"), ("inf_focus", "focus_distance must be finite and > 0")):
        assert lines[name][0] == "-1" and lines[name][1].startswith("lens: ") and words in lines[name][1], name
    assert lines["kept"] == lines["set"]  # a refused call changes nothing
    assert lines["off"][0] == "0" and _pair(lines["off"][1]) == (0.0, 3.0)
    assert lines["null"][0] == "-1" and "NULL scene" in lines["null"][1]
    assert lines["short"] == ["-4"] and lines["long"] == ["-4"]  # the pair is checked before it is read


def test_stubs_typecheck_and_agree_with_the_ml_file():
    subprocess.check_call(["gcc", "-std=gnu11", "-Wall", "-Wextra", "-Werror", "-fsyntax-only",
                           "-I", os.path.join(ROOT, "tests", "c", "mock_caml"), "-I", os.path.join(ROOT, "include"), "-I", B,
                           os.path.join(B, "ptx_stubs.c")])
    ml = open(os.path.join(B, "ptx.ml")).read()
    c = open(os.path.join(B, "ptx_stubs.c")).read()
    for stub, arity in (("ptx_ml_set_lens_stub", 2), ("ptx_ml_lens_stub", 1)):
        assert '"%s"' % stub in ml
        m = re.search(r"CAMLprim value %s\(([^)]*)\)" % stub, c)
        assert m and len(m.group(1).split(",")) == arity
        ext = re.search(r"external \w+\s*: ([^=]*)= \"%s\"" % stub, ml)
        assert ext and ext.group(1).count("->") == arity
    assert re.search(r"^let set_lens\b", ml, flags=re.M) and re.search(r"^external lens\b", ml, flags=re.M)
    assert "ptx_ml_set_lens(" in c and "ptx_ml_lens(" in c
    h = open(os.path.join(B, "ptx_ml_marshal.h")).read()
    assert "ptx_scene_set_lens(" in h and "ptx_scene_lens(" in h
