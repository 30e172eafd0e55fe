"""Progressive rendering at the C ABI, without a GPU: the three entry points (ptx_render_passes_device,
ptx_pixel_error_device, ptx_render_progressive) are declared, exported and mirrored; ptx_progressive_params has the layout
gcc gives it; every one of them refuses a host-only scene (there is no CPU fallback); the Python layer and the CLI reject bad
arguments before anything reaches a device."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("ptx_render_passes_device", "ptx_pixel_error_device", "ptx_render_progressive")


def test_new_entry_points_are_declared_exported_and_listed():
    import path_tracer_ocaml_amd as P
    hdr = open(os.path.join(ROOT, "include", "ptx.h")).read()
    L = P.lib()
    for name in NEW:
        assert f"{name}(" in hdr, name
        assert hasattr(L, name), name
        assert name in P.EXPORTS, name
    assert "typedef int32_t (*ptx_update_fn)(" in hdr
    assert L.ptx_version() == 6


def test_progressive_params_layout_matches_c(tmp_path):
    from path_tracer_ocaml_amd import abi
    src = tmp_path / "pp.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "ptx.h"\nint main(void){'
                   'printf("%zu %zu %zu %zu %zu\\n", sizeof(ptx_progressive_params), offsetof(ptx_progressive_params, passes_per_update),'
                   'offsetof(ptx_progressive_params, want_error), offsetof(ptx_progressive_params, target_rel_err),'
                   '_Alignof(ptx_progressive_params));return 0;}\n')
    exe = tmp_path / "pp"
    subprocess.check_call(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    T = abi.ProgressiveParams
    assert got == [C.sizeof(T), T.passes_per_update.offset, T.want_error.offset, T.target_rel_err.offset, C.alignment(T)]
    assert got[:4] == [16, 0, 4, 8]


@pytest.fixture
def host_only(oracle):
    import path_tracer_ocaml_amd as P
    d = oracle.desc_shirley(16, 12)
    s = P.Scene(d.ptr, -1, keepalive=d)
    yield P, s
    s.close()


def test_host_only_scene_refuses_every_new_entry_point(host_only):
    P, s = host_only
    params = P.render_params(16, 12, 4, 2)
    with pytest.raises(P.PtxError, match="no CPU fallback"):
        s.render_passes_device(params, 0, 2, 0)
    with pytest.raises(P.PtxError, match="no CPU fallback"):
        s.render_progressive(16, 12, 4, 2, passes_per_update=2)
    with pytest.raises(P.PtxError, match="no CPU fallback"):
        P.pixel_error_device(-1, 16, 12, 4, 0, 0)
    # the message is the library's own: nothing was attempted on a device
    assert "host-only" in P.last_error() or "no CPU fallback" in P.last_error()


def test_progressive_refusal_leaves_the_callers_buffers_alone(host_only):
    P, s = host_only
    out = np.full((12, 16, 3), 7.0)
    calls = []
    with pytest.raises(P.PtxError, match="no CPU fallback"):
        s.render_progressive(16, 12, 4, 2, passes_per_update=1, on_update=lambda *a: calls.append(a), out=out)
    assert not calls
    assert (out == 7.0).all()


@pytest.mark.parametrize("kw, match", [
    ({"passes_per_update": 0}, "passes_per_update"),
    ({"passes_per_update": -3}, "passes_per_update"),
    ({"passes_per_update": 2, "target_rel_err": -0.1}, "target_rel_err"),
    ({"passes_per_update": 2, "target_rel_err": float("nan")}, "target_rel_err"),
    ({"passes_per_update": 2, "target_rel_err": 0.01, "want_error": False}, "want_error"),
    ({"passes_per_update": 2, "want_error": False, "err_out": np.zeros((12, 16, 3))}, "want_error"),
    ({"passes_per_update": 2, "out": np.zeros((12, 16, 3), dtype=np.float32)}, "out"),
    ({"passes_per_update": 2, "out": np.zeros((16, 12, 3))}, "out"),
    ({"passes_per_update": 2, "err_out": np.zeros((12, 16, 3))[:, ::-1]}, "err_out"),
    ({"passes_per_update": 2, "n_gpus": 2}, "one GPU"),
])
def test_python_rejects_bad_progressive_arguments(host_only, kw, match):
    P, s = host_only
    with pytest.raises(ValueError, match=match):
        s.render_progressive(16, 12, 4, 2, **kw)


def _cli(*args):
    exe = os.path.join(ROOT, "path_tracer_ocaml_amd", "shirley_spheres")
    env = dict(os.environ)
    env["LD_LIBRARY_PATH"] = "/opt/rocm/lib:" + env.get("LD_LIBRARY_PATH", "")
    return subprocess.run([exe, "--dimension=16,8", "--no-progress", *args], capture_output=True, text=True, env=env, timeout=60)


@pytest.mark.parametrize("args, match", [
    (("--target-error=0.01",), "requires --progressive"),
    (("--progressive=0",), "--progressive"),
    (("--progressive=2", "--target-error=-1"), "--target-error"),
    (("--progressive=2", "--gpus=2"), "one GPU"),
])
def test_cli_rejects_bad_progressive_flags(args, match):
    """refused while parsing, before a scene exists: the reference's CLI error exit (Cmdliner's 124)"""
    r = _cli(*args)
    assert r.returncode == 124, (r.returncode, r.stderr)
    assert match in r.stderr
    assert r.stdout == ""


def test_cli_usage_lists_the_progressive_flags():
    r = _cli("--help")
    assert r.returncode == 0
    assert "--progressive=K" in r.stderr and "--target-error=FLOAT" in r.stderr
