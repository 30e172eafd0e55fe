"""Adaptive sampling at the C ABI, without a GPU: the four entry points (ptx_render_pixels_device, ptx_film_resolve_counts_device,
ptx_pixel_error_counts_device, ptx_render_adaptive) are declared, exported and mirrored; ptx_adaptive_params has the layout gcc
gives it; every one of them refuses a host-only scene (there is no CPU fallback); the Python layer and the CLI reject bad
arguments before anything reaches a device."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("ptx_render_pixels_device", "ptx_film_resolve_counts_device", "ptx_pixel_error_counts_device", "ptx_render_adaptive")


def test_new_entry_points_are_declared_exported_and_listed():
    import path_tracer_ocaml_amd as P
    hdr = open(os.path.join(ROOT, "include", "ptx.h")).read()
    L = P.lib()
    for name in NEW:
        assert f"{name}(" in hdr, name
        assert hasattr(L, name), name
        assert name in P.EXPORTS, name
    assert "typedef int32_t (*ptx_round_fn)(" in hdr
    assert L.ptx_version() == 6


def test_adaptive_params_layout_matches_c(tmp_path):
    from path_tracer_ocaml_amd import abi
    src = tmp_path / "ap.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "ptx.h"\nint main(void){'
                   'printf("%zu %zu %zu %zu %zu %zu\\n", sizeof(ptx_adaptive_params), offsetof(ptx_adaptive_params, min_passes),'
                   'offsetof(ptx_adaptive_params, passes_per_round), offsetof(ptx_adaptive_params, target_rel_err),'
                   'offsetof(ptx_adaptive_params, radiance_floor), _Alignof(ptx_adaptive_params));return 0;}\n')
    exe = tmp_path / "ap"
    subprocess.check_call(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    T = abi.AdaptiveParams
    assert got == [C.sizeof(T), T.min_passes.offset, T.passes_per_round.offset, T.target_rel_err.offset,
                   T.radiance_floor.offset, C.alignment(T)]
    assert got[:5] == [24, 0, 4, 8, 16]
    # the callback's C signature, argument for argument
    assert abi.ROUND_FN._restype_ is C.c_int32
    assert abi.ROUND_FN._argtypes_ == (C.c_void_p, C.c_int32, C.c_int32, C.c_int64, C.c_int64, C.c_double, C.c_void_p,
                                       C.c_void_p, C.c_void_p)


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
        s.render_pixels_device(params, 0, 2, 0, 0, 0)
    with pytest.raises(P.PtxError, match="no CPU fallback"):
        s.render_adaptive(16, 12, 4, 2, 0.01, min_passes=2, passes_per_round=1)
    with pytest.raises(P.PtxError, match="no CPU fallback"):
        P.film_resolve_counts_device(-1, 16, 12, 0, 0, 0)
    with pytest.raises(P.PtxError, match="no CPU fallback"):
        P.pixel_error_counts_device(-1, 16, 12, 0, 0, 0)
    assert "host-only" in P.last_error() or "no CPU fallback" in P.last_error()


def test_adaptive_refusal_leaves_the_callers_buffers_alone(host_only):
    P, s = host_only
    out, err, passes = np.full((12, 16, 3), 7.0), np.full((12, 16, 3), 5.0), np.full((12, 16), 3, dtype=np.int32)
    calls = []
    with pytest.raises(P.PtxError, match="no CPU fallback"):
        s.render_adaptive(16, 12, 4, 2, 0.01, min_passes=2, passes_per_round=1, on_round=lambda *a: calls.append(a), out=out,
                          err_out=err, passes_out=passes)
    assert not calls
    assert (out == 7.0).all() and (err == 5.0).all() and (passes == 3).all()


@pytest.mark.parametrize("kw, match", [
    ({"min_passes": 1}, "min_passes"),
    ({"min_passes": -2}, "min_passes"),
    ({"passes_per_round": 0}, "passes_per_round"),
    ({"target_rel_err": -0.1}, "target_rel_err"),
    ({"target_rel_err": float("nan")}, "target_rel_err"),
    ({"radiance_floor": -1e-3}, "radiance_floor"),
    ({"radiance_floor": float("nan")}, "radiance_floor"),
    ({"n_gpus": 2}, "one GPU"),
    ({"band_step": 2}, "one GPU"),
    ({"out": np.zeros((12, 16, 3), dtype=np.float32)}, "out"),
    ({"err_out": np.zeros((16, 12, 3))}, "err_out"),
    ({"passes_out": np.zeros((12, 16), dtype=np.int64)}, "passes_out"),
    ({"passes_out": np.zeros((12, 16, 1), dtype=np.int32)}, "passes_out"),
])
def test_python_rejects_bad_adaptive_arguments(host_only, kw, match):
    P, s = host_only
    args = {"target_rel_err": 0.01}
    args.update(kw)
    with pytest.raises(ValueError, match=match):
        s.render_adaptive(16, 12, 4, 2, **args)


def test_python_rejects_a_negative_list_length(host_only):
    P, s = host_only
    with pytest.raises(ValueError, match="n_pixels"):
        s.render_pixels_device(P.render_params(16, 12, 4, 2), 0, 2, 0, -1, 0)


def _cli(*args):
    exe = os.path.join(ROOT, "path_tracer_ocaml_amd", "shirley_spheres")
    env = dict(os.environ)
    env["LD_LIBRARY_PATH"] = "/opt/rocm/lib:" + env.get("LD_LIBRARY_PATH", "")
    return subprocess.run([exe, "--dimension=16,8", "--no-progress", *args], capture_output=True, text=True, env=env, timeout=60)


@pytest.mark.parametrize("args, match", [
    (("--adaptive=-0.5",), "--adaptive"),
    (("--adaptive=0.01", "--gpus=2"), "one GPU"),
    (("--adaptive=0.01", "--progressive=4", "--target-error=0.1"), "--target-error"),
    (("--min-passes=4",), "requires --adaptive"),
    (("--adaptive=0.01", "--min-passes=1"), "--min-passes"),
    (("--adaptive=0.01", "--progressive=0"), "--progressive"),
])
def test_cli_rejects_bad_adaptive_flags(args, match):
    """refused while parsing, before a scene exists: the reference's CLI error exit (Cmdliner's 124)"""
    r = _cli(*args)
    assert r.returncode == 124, (r.returncode, r.stderr)
    assert match in r.stderr
    assert r.stdout == ""


def test_cli_usage_lists_the_adaptive_flags():
    r = _cli("--help")
    assert r.returncode == 0
    assert "--adaptive=FLOAT" in r.stderr and "--min-passes=M" in r.stderr


def test_ocaml_binding_exposes_render_adaptive():
    b = os.path.join(ROOT, "bindings", "ocaml")
    ml = open(os.path.join(b, "ptx.ml")).read()
    assert "let render_adaptive" in ml and '"ptx_ml_render_adaptive_stub"' in ml
    assert "CAMLprim value ptx_ml_render_adaptive_stub(" in open(os.path.join(b, "ptx_stubs.c")).read()
    assert "ptx_render_adaptive(" in open(os.path.join(b, "ptx_ml_marshal.h")).read()
