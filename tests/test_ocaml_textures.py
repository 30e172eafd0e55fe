"""The OCaml binding's image functions (Ptx.set_texture_image / clear_texture_image / set_environment / clear_environment): the
marshalling the stubs delegate to (bindings/ocaml/ptx_ml_marshal.h) compiled and run from C against the real C ABI on a host-only
scene, and the stubs type-checked against the runtime's documented C interface (tests/c/mock_caml).  OCaml itself is not needed."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B = os.path.join(ROOT, "bindings", "ocaml")
LIBDIR = os.path.join(ROOT, "path_tracer_ocaml_amd")


@pytest.fixture(scope="module")
def lines(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("ocaml_textures") / "driver")
    subprocess.check_call(["gcc", "-O1", "-Wall", "-Werror", "-Wno-unused-function", "-I", os.path.join(ROOT, "include"), "-I", B,
                           os.path.join(ROOT, "tests", "c", "ocaml_texture_driver.c"), "-o", exe, "-L", LIBDIR, "-lptx_hip",
                           "-Wl,-rpath," + LIBDIR, "-Wl,-rpath-link,/opt/rocm/lib"])
    out = subprocess.check_output([exe], text=True)
    return {l.split()[0]: l.split(None, 2)[1:] for l in out.splitlines()}


def test_marshalling_drives_the_c_abi(lines):
    assert lines["set"] == ["0", "3 2 5"]           # bilinear | repeat v, as the getter answers
    assert lines["short"] == ["-4", "-"] and lines["null"] == ["-4", "-"]  # fewer texels than width * height * 3: nothing is read
    assert lines["kept"] == ["0", "3 2 5"]          # a refused call changes nothing
    assert lines["size"][0] == "-1" and "size 16385 x 1" in lines["size"][1]  # the library's own refusals keep their messages
    assert lines["flags"][0] == "-1" and "unknown bits in flags (0x8)" in lines["flags"][1]
    assert lines["index"][0] == "-1" and "texture index 2 out of range" in lines["index"][1]
    assert lines["texel"][0] == "-1" and "texel (2, 0) channel 1 is not finite" in lines["texel"][1]
    assert lines["clear"] == ["0", "0 0 0"]
    assert lines["env"] == ["0", "2 3 1 0 1 0"]     # R[0], R[2], R[8] of the rotation handed over
    assert lines["env_identity"] == ["0", "2 3 0 1 0 1"]
    assert lines["env_rot_len"] == ["-5", "-"] and lines["env_short"] == ["-4", "-"]
    assert lines["env_repeat"][0] == "-1" and "a repeat flag is not accepted" in lines["env_repeat"][1]
    assert lines["env_clear"] == ["0", "0 0 0 1 0 1"]


def test_stubs_typecheck_and_agree_with_the_ml_file():
    subprocess.check_call(["gcc", "-std=gnu11", "-Wall", "-Wextra", "-Werror", "-fsyntax-only",
                           "-I", os.path.join(ROOT, "tests", "c", "mock_caml"), "-I", os.path.join(ROOT, "include"), "-I", B,
                           os.path.join(B, "ptx_stubs.c")])
    ml = open(os.path.join(B, "ptx.ml")).read()
    c = open(os.path.join(B, "ptx_stubs.c")).read()
    for stub, arity in (("ptx_ml_set_texture_image_stub", 4), ("ptx_ml_set_environment_stub", 4)):
        assert '"%s"' % stub in ml
        m = re.search(r"CAMLprim value %s\(([^)]*)\)" % stub, c)
        assert m and len(m.group(1).split(",")) == arity  # at most 5 arguments: no bytecode twin is needed
        ext = re.search(r"external \w+ : ([^=]*)= \"%s\"" % stub, ml)
        assert ext and ext.group(1).count("->") == arity
    for name in ("set_texture_image", "clear_texture_image", "set_environment", "clear_environment"):
        assert re.search(r"^let %s\b" % name, ml, flags=re.M), name
    assert "ptx_scene_set_texture_image" in open(os.path.join(B, "ptx_ml_marshal.h")).read()
