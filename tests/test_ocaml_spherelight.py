"""The OCaml binding's sphere-light functions (Ptx.set_sphere_light_sampling / sphere_lights): the calls the stubs make, compiled and run
from C against the real C ABI on host-only scenes, and the stubs type-checked against the runtime's documented C interface
(tests/c/mock_caml).  OCaml itself is not needed."""
import math
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B = os.path.join(ROOT, "bindings", "ocaml")
LIBDIR = os.path.join(ROOT, "path_tracer_ocaml_amd")


@pytest.fixture(scope="module")
def lines(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("ocaml_spherelight") / "driver")
    subprocess.check_call(["gcc", "-O1", "-Wall", "-Werror", "-Wno-unused-function", "-I", os.path.join(ROOT, "include"), "-I", B,
                           os.path.join(ROOT, "tests", "c", "ocaml_spherelight_driver.c"), "-o", exe, "-L", LIBDIR, "-lptx_hip",
                           "-Wl,-rpath," + LIBDIR, "-Wl,-rpath-link,/opt/rocm/lib"])
    out = subprocess.check_output([exe], text=True, timeout=120)
    return {l.split()[0]: l.split(None, 2)[1:] for l in out.splitlines()}


def test_the_stub_calls_drive_the_c_abi(lines):
    assert lines["initial"] == ["0", "0 0 0x0p+0"]
    assert lines["dark"][0] == "-1" and "has 0" in lines["dark"][1]
    assert lines["lighting_refused"][0] == "-1" and "emissive triangle" in lines["lighting_refused"][1]
    rc, rest = lines["on"]
    on, n, total = rest.split()
    # one sphere of radius 0.5: W = 2 pi r^2
    assert (rc, on, n) == ("0", "1", "1") and math.isclose(float.fromhex(total), 2.0 * math.pi * 0.25, rel_tol=1e-15)
    assert lines["lighting"][0] == "0"
    assert lines["off_refused"][0] == "-3" and "lighting mode first" in lines["off_refused"][1]
    assert lines["kept"] == lines["on"]
    assert lines["path_order"][0] == "0" and lines["off"] == ["0", "0 0 0x0p+0"]


def test_stubs_typecheck_and_agree_with_the_ml_file():
    subprocess.check_call(["gcc", "-std=gnu11", "-Wall", "-Wextra", "-Werror", "-fsyntax-only",
                           "-I", os.path.join(ROOT, "tests", "c", "mock_caml"), "-I", os.path.join(ROOT, "include"), "-I", B,
                           os.path.join(B, "ptx_stubs.c")])
    ml = open(os.path.join(B, "ptx.ml")).read()
    c = open(os.path.join(B, "ptx_stubs.c")).read()
    for stub, arity in (("ptx_ml_set_sphere_light_sampling_stub", 2), ("ptx_ml_sphere_lights_stub", 1)):
        assert '"%s"' % stub in ml
        m = re.search(r"CAMLprim value %s\(([^)]*)\)" % stub, c)
        assert m and len(m.group(1).split(",")) == arity
        ext = re.search(r"external \w+ : ([^=]*)= \"%s\"" % stub, ml)
        assert ext and ext.group(1).count("->") == arity
    for name in ("set_sphere_light_sampling", "sphere_lights"):
        assert re.search(r"^let %s\b" % name, ml, flags=re.M), name
    assert "ptx_scene_set_sphere_light_sampling" in c and "ptx_scene_sphere_lights" in c
