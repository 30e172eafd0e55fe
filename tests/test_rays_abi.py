"""ptx_render_rays / ptx_render_rays_device without a GPU: the symbols, the struct as the C compiler sees it, and every refusal that
is decided before a device is touched, with its message.  A host-only scene (device -1) is enough: the caller's arguments are checked
first, and valid arguments then meet PTX_ERR_STATE."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import path_tracer_ocaml_amd as P
from path_tracer_ocaml_amd import abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PTX_ERR_ARG, PTX_ERR_STATE = -1, -3


@pytest.fixture(scope="module")
def scene(oracle):
    d = oracle.desc_shirley(16, 8)
    g = P.Scene(d.ptr, -1, keepalive=d)
    yield g
    g.close()


def _call(scene_handle, params, n, o, d, off, out, sq=None):
    dp, ip = abi.c_double_p, abi.c_int32_p
    return P.lib().ptx_render_rays(scene_handle, None if params is None else C.byref(params), n,
                                   None if o is None else o.ctypes.data_as(dp), None if d is None else d.ctypes.data_as(dp),
                                   None if off is None else off.ctypes.data_as(ip), None if out is None else out.ctypes.data_as(dp),
                                   None if sq is None else sq.ctypes.data_as(dp), None)


def _rays(n=6):
    return np.zeros((n, 3)), np.tile([0.0, 0.0, -1.0], (n, 1)), np.zeros((n, 3))


def test_the_symbols_exist():
    L = P.lib()
    assert "ptx_render_rays" in P.EXPORTS and "ptx_render_rays_device" in P.EXPORTS
    assert L.ptx_render_rays and L.ptx_render_rays_device
    assert L.ptx_version() == 6  # only entry points, one struct and a define were added


def test_the_struct_is_16_bytes_in_c_and_in_python(tmp_path):
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "ptx.h"\nint main(void){'
                   'printf("%zu %zu %zu %zu %zu %d\\n", sizeof(ptx_rays_params), offsetof(ptx_rays_params, max_bounces),'
                   'offsetof(ptx_rays_params, rays_per_bin), offsetof(ptx_rays_params, flags), offsetof(ptx_rays_params, count_work),'
                   'PTX_RAYS_NORMALIZE);return 0;}\n')
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    R = abi.RaysParams
    assert got == [16, 0, 4, 8, 12, 1]
    assert [C.sizeof(R), R.max_bounces.offset, R.rays_per_bin.offset, R.flags.offset, R.count_work.offset, abi.PTX_RAYS_NORMALIZE] == got
    p = abi.rays_params(5, 3, normalize=True, count_work=True)
    assert (p.max_bounces, p.rays_per_bin, p.flags, p.count_work) == (5, 3, 1, 1)


def test_a_host_only_scene_is_a_state_error(scene):
    o, d, out = _rays()
    assert _call(scene._h, abi.rays_params(4), 6, o, d, None, out) == PTX_ERR_STATE
    assert "host-only" in P.last_error()
    assert _call(scene._h, abi.rays_params(4), 0, o, d, None, out) == PTX_ERR_STATE  # the scene's state comes before n == 0
    assert P.lib().ptx_render_rays_device(scene._h, C.byref(abi.rays_params(4)), 6, 8, 8, None, 8, None, None, None) == PTX_ERR_STATE
    with pytest.raises(P.PtxError, match="host-only"):
        scene.render_rays(o, d, max_bounces=4)
    with pytest.raises(P.PtxError, match="host-only"):
        scene.render_rays_device(6, 8, 8, 8)


@pytest.mark.parametrize("what, words", [
    ("null_scene", "NULL scene"), ("null_params", "NULL params"), ("null_origins", "NULL argument"), ("null_directions", "NULL argument"),
    ("null_sums", "NULL argument"), ("depth_low", "max_bounces must be in [0, 126]"), ("depth_high", "max_bounces must be in [0, 126]"),
    ("bin_zero", "rays_per_bin must be >= 1"), ("bin_negative", "rays_per_bin must be >= 1"), ("flags", "unknown bits in flags"),
    ("n_negative", "bad ray count"), ("n_2_31", "bad ray count"), ("n_not_multiple", "is not a multiple of rays_per_bin = 4")])
def test_argument_refusals_name_the_rule(scene, what, words):
    o, d, out = _rays()
    h, p, n = scene._h, abi.rays_params(4), 6
    if what == "null_scene":
        h = None
    elif what == "null_params":
        p = None
    elif what == "null_origins":
        o = None
    elif what == "null_directions":
        d = None
    elif what == "null_sums":
        out = None
    elif what == "depth_low":
        p.max_bounces = -1
    elif what == "depth_high":
        p.max_bounces = 127
    elif what == "bin_zero":
        p.rays_per_bin = 0
    elif what == "bin_negative":
        p.rays_per_bin = -3
    elif what == "flags":
        p.flags = 2
    elif what == "n_negative":
        n = -1
    elif what == "n_2_31":
        n = 2**31 - 1
    elif what == "n_not_multiple":
        p.rays_per_bin = 4
    assert _call(h, p, n, o, d, None, out) == PTX_ERR_ARG
    assert words in P.last_error(), P.last_error()
    if out is not None:
        assert not out.any()  # nothing was written


def test_the_device_call_checks_the_same_arguments(scene):
    L = P.lib()
    p = abi.rays_params(4, 4)
    assert L.ptx_render_rays_device(scene._h, C.byref(p), 6, 8, 8, None, 8, None, None, None) == PTX_ERR_ARG
    assert "is not a multiple of rays_per_bin = 4" in P.last_error()
    assert L.ptx_render_rays_device(scene._h, C.byref(abi.rays_params(4)), 6, 8, 8, None, None, None, None, None) == PTX_ERR_ARG
    assert "NULL argument" in P.last_error()


def test_the_wrapper_refuses_mismatched_arrays(scene):
    o, d, _ = _rays()
    with pytest.raises(ValueError, match="differ in shape"):
        scene.render_rays(o, d[:3])
    with pytest.raises(ValueError, match="offsets for 6 rays"):
        scene.render_rays(o, d, offsets=[0, 1])
    with pytest.raises(ValueError, match="32 bits"):
        scene.render_rays(o, d, offsets=[0, 1, 2, 3, 4, 2**31])
