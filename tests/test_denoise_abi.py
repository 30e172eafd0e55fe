"""The feature buffers and the denoiser at the C ABI, without a GPU: the four entry points (ptx_render_features_device,
ptx_denoise_defaults, ptx_denoise_device, ptx_render_denoised) are declared, exported and mirrored; ptx_denoise_params has the
layout gcc gives it; every compute call refuses a host-only scene or device -1 (there is no CPU fallback) and leaves the caller's
buffers alone; the Python layer and the CLI reject bad arguments before anything reaches a device."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("ptx_render_features_device", "ptx_denoise_defaults", "ptx_denoise_device", "ptx_render_denoised")


def test_new_entry_points_are_declared_exported_and_listed():
    import path_tracer_ocaml_amd as P
    hdr = open(os.path.join(ROOT, "include", "ptx.h")).read()
    L = P.lib()
    for name in NEW:
        assert f"{name}(" in hdr, name
        assert hasattr(L, name), name
        assert name in P.EXPORTS, name
        assert getattr(L, name).argtypes, name
    assert "#define PTX_FEATURE_DOUBLES 8" in hdr and "#define PTX_DENOISE_DEMODULATE 1" in hdr
    assert "#define PTX_ABI_VERSION 6" in hdr
    assert L.ptx_version() == 6
    for name in ("denoise_defaults", "denoise_device"):
        assert callable(getattr(P, name))
    for name in ("render_features_device", "render_denoised"):
        assert callable(getattr(P.Scene, name))
    from path_tracer_ocaml_amd.integrator import Integrator
    assert callable(Integrator.render_denoised)


def test_denoise_params_layout_matches_c(tmp_path):
    from path_tracer_ocaml_amd import abi
    fields = ("levels", "normal_power_log2", "feature_passes", "flags", "sigma_luminance", "sigma_depth", "sigma_albedo")
    src = tmp_path / "dp.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "ptx.h"\nint main(void){'
                   'printf("%zu %zu", sizeof(ptx_denoise_params), _Alignof(ptx_denoise_params));'
                   + "".join(f'printf(" %zu", offsetof(ptx_denoise_params, {f}));' for f in fields)
                   + 'printf(" %d %d\\n", PTX_FEATURE_DOUBLES, PTX_DENOISE_DEMODULATE);return 0;}\n')
    exe = tmp_path / "dp"
    subprocess.check_call(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    T = abi.DenoiseParams
    assert got == [C.sizeof(T), C.alignment(T)] + [getattr(T, f).offset for f in fields] + [abi.PTX_FEATURE_DOUBLES,
                                                                                              abi.PTX_DENOISE_DEMODULATE]
    assert got[0] == 40 and got[2:9] == [0, 4, 8, 12, 16, 24, 32]


def test_defaults_are_the_documented_ones():
    import path_tracer_ocaml_amd as P
    d = P.denoise_defaults()
    assert (d.levels, d.normal_power_log2, d.feature_passes, d.flags) == (5, 5, 8, 1)
    assert (d.sigma_luminance, d.sigma_depth, d.sigma_albedo) == (4.0, 0.05, 0.2)
    assert P.lib().ptx_denoise_defaults(None) == -1
    import denoise_reference as R
    assert R.DEFAULTS == {f: getattr(d, f) for f, _ in type(d)._fields_}


@pytest.fixture
def host_only(oracle):
    import path_tracer_ocaml_amd as P
    d = oracle.desc_shirley(16, 12)
    s = P.Scene(d.ptr, -1, keepalive=d)
    yield P, s
    s.close()


def test_no_cpu_fallback_and_the_callers_buffers_stay_untouched(host_only):
    P, s = host_only
    params = P.render_params(16, 12, 4, 2)
    with pytest.raises(P.PtxError, match="no CPU fallback"):
        s.render_features_device(params, 0, 2, 0)
    with pytest.raises(P.PtxError, match="no CPU fallback"):
        P.denoise_device(-1, 16, 12, None, 4, 2, 0, 0, 0, 0)
    out, err, feat = np.full((12, 16, 3), 7.0), np.full((12, 16, 3), 5.0), np.full((12, 16, 8), 3.0)
    calls = []
    with pytest.raises(P.PtxError, match="no CPU fallback"):
        s.render_denoised(16, 12, 4, 2, 2, on_update=lambda *a: calls.append(a), out=out, err_out=err, feat_out=feat)
    assert not calls
    assert (out == 7.0).all() and (err == 5.0).all() and (feat == 3.0).all()
    from path_tracer_ocaml_amd.integrator import Integrator
    image = np.full((12, 16, 3), 9.0)
    integ = Integrator.create(width=16, height=12, image=image, samples_per_pixel=4, max_bounces=2, scene=s)
    with pytest.raises(P.PtxError, match="no CPU fallback"):
        integ.render_denoised(2)
    assert (image == 9.0).all()


@pytest.mark.parametrize("kw, match", [
    ({"denoise": {"levels": 9}}, "levels"),
    ({"denoise": {"levels": -1}}, "levels"),
    ({"denoise": {"normal_power_log2": -1}}, "normal_power_log2"),
    ({"denoise": {"normal_power_log2": 9}}, "normal_power_log2"),
    ({"denoise": {"feature_passes": -1}}, "feature_passes"),
    ({"denoise": {"sigma_luminance": 0.0}}, "sigma_luminance"),
    ({"denoise": {"sigma_depth": -1.0}}, "sigma_depth"),
    ({"denoise": {"sigma_albedo": float("nan")}}, "sigma_albedo"),
    ({"denoise": {"sigma_albedo": float("inf")}}, "sigma_albedo"),
    ({"denoise": {"flags": 2}}, "flags"),
    ({"denoise": {"sigma": 1.0}}, "unknown denoiser setting"),
    ({"passes_per_update": 1}, "passes_per_update"),
    ({"samples_per_pixel": 1}, "samples_per_pixel"),
    ({"target_rel_err": -0.5}, "target_rel_err"),
    ({"n_gpus": 2}, "one GPU"),
    ({"band_step": 2}, "one GPU"),
    ({"out": np.zeros((12, 16, 3), dtype=np.float32)}, "out"),
    ({"err_out": np.zeros((16, 12, 3))}, "err_out"),
    ({"feat_out": np.zeros((12, 16, 3))}, "feat_out"),
    ({"feat_out": np.zeros((12, 16, 8), dtype=np.float32)}, "feat_out"),
])
def test_python_rejects_bad_render_denoised_arguments(host_only, kw, match):
    P, s = host_only
    args = {"samples_per_pixel": 4, "passes_per_update": 2}
    args.update(kw)
    spp, k = args.pop("samples_per_pixel"), args.pop("passes_per_update")
    with pytest.raises(ValueError, match=match):
        s.render_denoised(16, 12, spp, 2, k, **args)


def test_python_rejects_bad_device_call_arguments(host_only):
    P, s = host_only
    with pytest.raises(ValueError, match="one GPU"):
        s.render_features_device(P.render_params(16, 12, 4, 2, n_gpus=2), 0, 1, 0)
    with pytest.raises(ValueError, match="one GPU"):
        s.render_features_device(P.render_params(16, 12, 4, 2, band_step=2), 0, 1, 0)
    with pytest.raises(ValueError, match="passes_done"):
        P.denoise_device(0, 16, 12, None, 1, 1, 0, 0, 0, 0)
    with pytest.raises(ValueError, match="feature_passes_done"):
        P.denoise_device(0, 16, 12, None, 4, 0, 0, 0, 0, 0)
    with pytest.raises(ValueError, match="levels"):
        P.denoise_device(0, 16, 12, {"levels": 9}, 4, 2, 0, 0, 0, 0)
    with pytest.raises(ValueError, match="dimensions"):
        P.denoise_device(0, 0, 12, None, 4, 2, 0, 0, 0, 0)


def test_the_library_checks_the_same_arguments(host_only):
    """behind the Python layer: the C entry points refuse them too (NULL pointers and a host-only scene come first)"""
    P, s = host_only
    L = P.lib()
    dn = P.denoise_defaults()
    assert L.ptx_denoise_device(-1, 16, 12, C.byref(dn), 4, None, 2, None, None, None, None, None) == -3
    assert L.ptx_denoise_device(0, 16, 12, C.byref(dn), 4, None, 2, None, None, None, None, None) == -1  # NULL buffers
    assert L.ptx_render_features_device(None, None, 0, 1, None, None, None) == -1
    assert L.ptx_render_denoised(None, None, None, None, None, None, None, None, None, None, None) == -1


def _cli(*args):
    exe = os.path.join(ROOT, "path_tracer_ocaml_amd", "shirley_spheres")
    env = dict(os.environ)
    env["LD_LIBRARY_PATH"] = "/opt/rocm/lib:" + env.get("LD_LIBRARY_PATH", "")
    return subprocess.run([exe, "--dimension=16,8", "--no-progress", *args], capture_output=True, text=True, env=env, timeout=60)


@pytest.mark.parametrize("args, match", [
    (("--denoise", "--samples-per-pixel=8", "--adaptive=0.01"), "--denoise cannot be combined with --adaptive"),
    (("--denoise", "--samples-per-pixel=8", "--gpus=2"), "--denoise renders on one GPU"),
    (("--denoise=9", "--samples-per-pixel=8"), "invalid value for --denoise, LEVELS must be in 0..8"),
    (("--denoise=-1", "--samples-per-pixel=8"), "invalid value for --denoise, LEVELS must be in 0..8"),
    (("--denoise=x", "--samples-per-pixel=8"), "invalid value for --denoise, LEVELS must be in 0..8"),
    (("--aov=out", "--samples-per-pixel=8"), "--aov requires --denoise"),
    (("--denoise",), "--denoise requires --samples-per-pixel >= 2"),
    (("--denoise", "--samples-per-pixel=8", "--progressive=1"), "--denoise requires --progressive >= 2"),
])
def test_cli_rejects_bad_denoise_flags(args, match):
    """refused while parsing, before a scene exists: the reference's CLI error exit (Cmdliner's 124)"""
    r = _cli(*args)
    assert r.returncode == 124, (r.returncode, r.stderr)
    assert match in r.stderr
    assert r.stdout == ""


def test_cli_usage_lists_the_denoise_flags():
    r = _cli("--help")
    assert r.returncode == 0
    assert "--denoise[=LEVELS]" in r.stderr and "--aov=PREFIX" in r.stderr


def test_ocaml_binding_exposes_render_denoised():
    b = os.path.join(ROOT, "bindings", "ocaml")
    ml = open(os.path.join(b, "ptx.ml")).read()
    assert "let render_denoised" in ml and '"ptx_ml_render_denoised_stub"' in ml
    assert "CAMLprim value ptx_ml_render_denoised_stub(" in open(os.path.join(b, "ptx_stubs.c")).read()
    assert "ptx_render_denoised(" in open(os.path.join(b, "ptx_ml_marshal.h")).read()
