"""The OCaml binding's ray and projection functions (Ptx.render_rays / Ptx.set_camera_projection / Ptx.camera_projection): the calls
the stubs make, compiled and run from C against the real C ABI on a host-only scene, and the stubs type-checked against the runtime's
documented C interface (tests/c/mock_caml).  OCaml itself is not needed."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B = os.path.join(ROOT, "bindings", "ocaml")
LIBDIR = os.path.join(ROOT, "path_tracer_ocaml_amd")


@pytest.fixture(scope="module")
def lines(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("ocaml_rays") / "driver")
    subprocess.check_call(["gcc", "-O1", "-Wall", "-Werror", "-Wno-unused-function", "-I", os.path.join(ROOT, "include"), "-I", B,
                           os.path.join(ROOT, "tests", "c", "ocaml_rays_driver.c"), "-o", exe, "-L", LIBDIR, "-lptx_hip",
                           "-Wl,-rpath," + LIBDIR, "-Wl,-rpath-link,/opt/rocm/lib"])
    out = subprocess.check_output([exe], text=True)
    return {l.split()[0]: l.split(None, 2)[1:] for l in out.splitlines()}


def test_the_projection_calls_drive_the_c_abi(lines):
    assert lines["initial"] == ["0", "0"] and lines["latlong"] == ["0", "1"]
    assert lines["unknown"][0] == "-1" and lines["unknown"][1].startswith("camera projection: ")
    assert lines["kept"] == ["0", "1"]  # a refused call changes nothing
    assert lines["lens_under_latlong"][0] == "-3" and "PTX_PROJECTION_PERSPECTIVE) first" in lines["lens_under_latlong"][1]
    assert lines["perspective"] == ["0", "0"] and lines["lens"] == ["0", "0"]
    assert lines["latlong_under_lens"][0] == "-3" and "ptx_scene_set_lens(scene, 0, 1) first" in lines["latlong_under_lens"][1]
    assert lines["lens_off"] == ["0", "0"]
    assert lines["null"][0] == "-1" and "NULL scene" in lines["null"][1] and lines["null_get"] == ["-1"]


def test_the_ray_call_checks_lengths_first_and_then_reaches_the_library(lines):
    for name in ("ragged_origins", "short_directions", "short_offsets", "short_sums", "long_sums_for_bins", "short_squares"):
        assert lines[name] == ["-4"], name
    for name in ("host_only", "host_only_bins"):  # valid arrays: the library's own answer for a scene without a device
        assert lines[name][0] == "-3" and "host-only" in lines[name][1], name
    assert lines["not_a_multiple"][0] == "-1" and "is not a multiple of rays_per_bin = 3" in lines["not_a_multiple"][1]
    assert lines["zero_bin"][0] == "-1" and "rays_per_bin must be >= 1" in lines["zero_bin"][1]
    assert lines["touched"] == ["0"]


def test_stubs_typecheck_and_agree_with_the_ml_file():
    subprocess.check_call(["gcc", "-std=gnu11", "-Wall", "-Wextra", "-Werror", "-fsyntax-only",
                           "-I", os.path.join(ROOT, "tests", "c", "mock_caml"), "-I", os.path.join(ROOT, "include"), "-I", B,
                           os.path.join(B, "ptx_stubs.c")])
    ml = open(os.path.join(B, "ptx.ml")).read()
    c = open(os.path.join(B, "ptx_stubs.c")).read()
    for stub, arity in (("ptx_ml_set_camera_projection_stub", 2), ("ptx_ml_camera_projection_stub", 1), ("ptx_ml_render_rays_stub", 7)):
        assert '"%s"' % stub in ml
        m = re.search(r"CAMLprim value %s\(([^)]*)\)" % stub, c)
        assert m and len(m.group(1).split(",")) == arity
        ext = re.search(r"external \w+\s*:((?:[^=\"]|\(\*.*?\*\))*)=(?: \"\w+\")? \"%s\"" % stub, ml, flags=re.S)
        assert ext, stub
        assert re.sub(r"\(\*.*?\*\)", "", ext.group(1), flags=re.S).count("->") == arity, stub
    assert '"ptx_ml_render_rays_stub_bytecode" "ptx_ml_render_rays_stub"' in ml  # more than five arguments: a bytecode entry too
    assert "CAMLprim value ptx_ml_render_rays_stub_bytecode(value* argv, int argn)" in c
    for name in ("set_camera_projection", "camera_projection", "render_rays"):
        assert re.search(r"^let %s\b" % name, ml, flags=re.M)
    assert ml.index("let render_rays") > ml.index("external render_rays_flat")
    assert "FA." not in ml[:ml.index("module FA")]  # nothing uses the alias before it is defined
    h = open(os.path.join(B, "ptx_ml_marshal.h")).read()
    assert "ptx_scene_set_camera_projection(" in h and "ptx_scene_camera_projection(" in h and "ptx_render_rays(" in h
