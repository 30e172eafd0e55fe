"""Display outputs at the C ABI, without a GPU: the struct's layout against the ctypes mirror, the defines, the declared symbols
exported and listed, the Python surface; ptx_version() stays 6."""
import ctypes as C
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("ptx_display_defaults", "ptx_display_check", "ptx_display_pixel_bytes", "ptx_display_thresholds", "ptx_display_apply",
       "ptx_display_image_device", "ptx_display_range_device", "ptx_image_pin_bytes", "ptx_render_display", "ptx_render_progressive_display")
DEFINES = ("PTX_PIXEL_RGB8", "PTX_PIXEL_RGBA8", "PTX_PIXEL_RGB32F", "PTX_PIXEL_RGBA32F", "PTX_TRANSFER_REFERENCE",
           "PTX_TRANSFER_LINEAR", "PTX_TRANSFER_SRGB", "PTX_TONE_NONE", "PTX_TONE_REINHARD", "PTX_TONE_ACES")


def test_new_entry_points_are_declared_exported_and_listed():
    import path_tracer_ocaml_amd as P
    from path_tracer_ocaml_amd import integrator
    hdr = open(os.path.join(ROOT, "include", "ptx.h")).read()
    L = P.lib()
    for name in NEW:
        assert f"{name}(" in hdr, name
        assert hasattr(L, name), name
        assert name in P.EXPORTS, name
        assert getattr(L, name).argtypes, name
    assert "#define PTX_ABI_VERSION 6" in hdr
    assert L.ptx_version() == 6
    for f in (P.display_defaults, P.display_thresholds, P.display_apply, P.display_image_device, P.display_pixel_bytes,
              P.Scene.render_display, P.Scene.render_progressive_display, P.Scene.image_pin_bytes,
              integrator.Integrator.render_display, integrator.Integrator.render_progressive_display):
        assert callable(f)


def test_display_params_layout_and_defines_match_c(tmp_path):
    from path_tracer_ocaml_amd import abi
    fields = ("format", "transfer", "tone", "flags", "exposure", "reserved")
    src = tmp_path / "dp.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "ptx.h"\nint main(void){'
                   'printf("%zu %zu", sizeof(ptx_display_params), _Alignof(ptx_display_params));'
                   + "".join(f'printf(" %zu", offsetof(ptx_display_params, {f}));' for f in fields)
                   + 'printf(" %zu", sizeof(((ptx_display_params*)0)->reserved));'
                   + "".join(f'printf(" %d", {d});' for d in DEFINES) + 'printf("\\n");return 0;}\n')
    exe = tmp_path / "dp"
    subprocess.check_call(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    T = abi.DisplayParams
    want = [C.sizeof(T), C.alignment(T)] + [getattr(T, f).offset for f in fields] + [C.sizeof(C.c_int32 * 4)] + \
        [getattr(abi, d) for d in DEFINES]
    assert got == want
    assert C.sizeof(T) == 40
    assert abi.PTX_PIXEL_NAMES == ("rgb8", "rgba8", "rgb32f", "rgba32f")
    assert abi.PTX_TRANSFER_NAMES == ("reference", "linear", "srgb") and abi.PTX_TONE_NAMES == ("none", "reinhard", "aces")
