"""The temporal entry points without a GPU: the symbols, the struct sizes against the C compiler, the defaults, every refused
setting and camera with its message, the NULL and aliased buffers, and the refusals of a host-only scene -- all decided before a
device is touched, so fake device addresses are enough (nothing dereferences them)."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

import path_tracer_ocaml_amd as P
from path_tracer_ocaml_amd import abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PTX_ERR_ARG, PTX_ERR_STATE = -1, -3
W, H = 8, 4
NAMES = ("ptx_temporal_defaults", "ptx_temporal_accumulate_device", "ptx_render_temporal", "ptx_temporal_reset")
VIEW = (-1.0, -0.5, 2.0, 1.0)


def test_the_symbols_exist():
    L = P.lib()
    header = open(os.path.join(ROOT, "include", "ptx.h")).read()
    for name in NAMES:
        assert name in P.EXPORTS and getattr(L, name) and f"int32_t {name}(" in header, name
    assert L.ptx_version() == 6  # only entry points and structs were added


def test_struct_sizes_match_c(tmp_path):
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "ptx.h"\nint main(void){'
                   'printf("%zu %zu %zu %zu %d\\n", sizeof(ptx_temporal_camera), sizeof(ptx_temporal_params),'
                   'offsetof(ptx_temporal_camera, rotation), offsetof(ptx_temporal_camera, view), PTX_HISTORY_DOUBLES);return 0;}\n')
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    assert got == [128, 32, 24, 96, 12]
    assert got == [C.sizeof(abi.TemporalCamera), C.sizeof(abi.TemporalParams), abi.TemporalCamera.rotation.offset,
                   abi.TemporalCamera.view.offset, abi.PTX_HISTORY_DOUBLES]


def test_the_defaults():
    t = P.temporal_defaults()
    assert (t.max_history_passes, t.normal_threshold, t.depth_tolerance, t.min_weight) == (64.0, 0.9, 0.02, 2.0 ** -10)
    assert P.lib().ptx_temporal_defaults(None) == PTX_ERR_ARG


def _camera(origin=(0.0, 0.0, 0.0), rotation=None, view=VIEW):
    return abi.temporal_camera(origin, np.eye(3) if rotation is None else rotation, view)


# fake, distinct, 16-byte aligned device addresses, far enough apart for a W x H frame: no refusal below dereferences one
ADDR = {name: 0x10000000 + 0x100000 * i for i, name in enumerate(("raw", "sq", "feat", "hist_prev", "hist_out", "raw_out", "err_out", "motion"))}


def _call(temporal=None, k=4, kf=4, cur="ok", prev="ok", device=0, w=W, h=H, **addr):
    a = dict(ADDR, **addr)
    null_settings = isinstance(temporal, str)
    t = P.temporal_defaults() if temporal is None or null_settings else temporal
    cur = _camera() if cur == "ok" else cur
    prev = _camera() if prev == "ok" else prev
    vp = lambda v: C.c_void_p(v) if v else None  # noqa: E731
    took = C.c_int64(-7)
    rc = P.lib().ptx_temporal_accumulate_device(device, w, h, None if null_settings else C.byref(t), k, kf, C.byref(cur) if cur is not None else None,
                                                C.byref(prev) if prev is not None else None, vp(a["raw"]), vp(a["sq"]), vp(a["feat"]),
                                                vp(a["hist_prev"]), vp(a["hist_out"]), vp(a["raw_out"]), vp(a["err_out"]), vp(a["motion"]),
                                                C.byref(took), None)
    assert took.value == -7  # a refused call writes nothing
    return rc, P.last_error()


BAD_SETTINGS = [
    (dict(max_history_passes=-1.0), "max_history_passes must be >= 0"), (dict(max_history_passes=math.nan), "must be finite"),
    (dict(max_history_passes=math.inf), "must be finite"),
    (dict(normal_threshold=1.5), "normal_threshold must be in [-1, 1]"), (dict(normal_threshold=-1.0001), "normal_threshold must be in [-1, 1]"),
    (dict(normal_threshold=math.nan), "must be finite"),
    (dict(depth_tolerance=-1e-9), "depth_tolerance must be >= 0"), (dict(depth_tolerance=math.inf), "must be finite"),
    (dict(min_weight=1.0), "min_weight must be in [0, 1)"), (dict(min_weight=-0.5), "min_weight must be in [0, 1)"),
    (dict(min_weight=math.nan), "must be finite"),
]


@pytest.mark.parametrize("change, words", BAD_SETTINGS)
def test_refused_settings(change, words):
    t = P.temporal_defaults()
    for k, v in change.items():
        setattr(t, k, v)
    rc, msg = _call(temporal=t)
    assert rc == PTX_ERR_ARG and msg.startswith("temporal: ") and words in msg, msg
    with pytest.raises(ValueError):
        P.temporal_params(change)


def test_accepted_edges_of_the_settings_reach_the_device_check():
    """cap 0, threshold -1 and 1, tolerance 0, min_weight 0: accepted -- the call goes on to look for its device.
    Runs only where there is no HIP device: with one, the call would go on to read the fake device addresses.  On a GPU the accepted
    edges are covered by tests/test_gpu_temporal.py (test_other_settings_equal_the_restatement)."""
    if P.lib().ptx_device_count() > 0:
        pytest.skip("a HIP device is present: the fake addresses would be used")
    for change in (dict(max_history_passes=0.0), dict(normal_threshold=-1.0), dict(normal_threshold=1.0), dict(depth_tolerance=0.0), dict(min_weight=0.0)):
        t = P.temporal_params(change)
        rc, msg = _call(temporal=t)
        assert rc == PTX_ERR_ARG and "no CPU fallback" in msg, msg


def _rot(angle=0.3):
    c, s = math.cos(angle), math.sin(angle)
    return np.array([[c, 0.0, s], [0.0, 1.0, 0.0], [-s, 0.0, c]])


BAD_CAMERAS = [
    (dict(origin=(math.nan, 0.0, 0.0)), "origin must be finite"), (dict(origin=(0.0, math.inf, 0.0)), "origin must be finite"),
    (dict(rotation=np.full((3, 3), math.nan)), "rotation must be finite"),
    (dict(rotation=_rot() * (1.0 + 1e-8)), "max |R R^T - I|"), (dict(rotation=np.diag([1.0, 1.0, -1.0])), "det R > 0"),
    (dict(view=(math.nan, -0.5, 2.0, 1.0)), "view must be finite"), (dict(view=(-1.0, -0.5, math.inf, 1.0)), "view must be finite"),
    (dict(view=(-1.0, -0.5, 0.0, 1.0)), "view_x and view_y"), (dict(view=(-1.0, -0.5, 2.0, -0.0)), "view_x and view_y"),
]


@pytest.mark.parametrize("which", ["cur", "prev"])
@pytest.mark.parametrize("change, words", BAD_CAMERAS)
def test_refused_cameras(which, change, words):
    rc, msg = _call(**{which: _camera(**change)})
    assert rc == PTX_ERR_ARG and words in msg, msg
    if "view_x" in words:
        assert ("current" if which == "cur" else "previous") in msg, msg


def test_a_previous_camera_is_not_read_without_a_history():
    """Runs only where there is no HIP device, for the same reason; on a GPU the NULL-history camera pair of
    tests/test_gpu_temporal.py passes a NULL previous camera to the device function."""
    if P.lib().ptx_device_count() > 0:
        pytest.skip("a HIP device is present: the fake addresses would be used")
    rc, msg = _call(prev=None, hist_prev=0)
    assert rc == PTX_ERR_ARG and "no CPU fallback" in msg, msg  # accepted up to the device check


def test_null_aliased_and_counted_arguments():
    for name in ("raw", "sq", "feat", "hist_out", "raw_out", "err_out"):
        rc, msg = _call(**{name: 0})
        assert rc == PTX_ERR_ARG and "NULL argument" in msg, (name, msg)
    assert _call(temporal="null")[0] == PTX_ERR_ARG and _call(cur=None)[0] == PTX_ERR_ARG
    rc, msg = _call(prev=None)  # a history without its camera
    assert rc == PTX_ERR_ARG and "prev_camera may be NULL only with a NULL history" in msg
    rc, msg = _call(hist_out=ADDR["hist_prev"])
    assert rc == PTX_ERR_ARG and "d_hist_prev and d_hist_out must not alias" in msg, msg
    rc, msg = _call(raw_out=ADDR["raw"])
    assert rc == PTX_ERR_ARG and "d_raw and d_raw_out must not alias" in msg, msg
    rc, msg = _call(err_out=ADDR["raw_out"] + 8)  # overlapping, not equal
    assert rc == PTX_ERR_ARG and "must not alias" in msg, msg
    rc, msg = _call(motion=ADDR["sq"])
    assert rc == PTX_ERR_ARG and "d_sq and d_motion_out must not alias" in msg, msg
    rc, msg = _call(hist_out=ADDR["hist_out"] + 8)
    assert rc == PTX_ERR_ARG and "16-byte aligned" in msg, msg
    for k, kf, words in ((1, 4, "passes_done must be >= 2"), (0, 4, "passes_done must be >= 2"), (4, 0, "feature_passes_done must be >= 1")):
        rc, msg = _call(k=k, kf=kf)
        assert rc == PTX_ERR_ARG and words in msg, msg
    for w, h in ((0, 4), (8, -1)):
        assert _call(w=w, h=h)[0] == PTX_ERR_ARG
    rc, msg = _call(device=-1)
    assert rc == PTX_ERR_STATE and "no CPU fallback" in msg


def test_a_host_only_scene_is_refused(oracle):
    d = oracle.desc_shirley(16, 8)
    g = P.Scene(d.ptr, -1, keepalive=d)
    with pytest.raises(P.PtxError, match="host-only"):
        g.render_temporal(16, 8, 16, 4, 0, 4)
    p, t, out = P.render_params(16, 8, 16, 4), P.temporal_defaults(), np.zeros((8, 16, 3))
    rc = P.lib().ptx_render_temporal(g._h, C.byref(p), C.byref(t), None, 0, 4, out.ctypes.data_as(abi.c_double_p), None, None, None, None)
    assert rc == PTX_ERR_STATE and "host-only" in P.last_error()
    g.temporal_reset()  # accepted: there is nothing to drop
    assert P.lib().ptx_temporal_reset(None) == PTX_ERR_ARG and "NULL scene" in P.last_error()
    assert P.lib().ptx_render_temporal(None, C.byref(p), C.byref(t), None, 0, 4, out.ctypes.data_as(abi.c_double_p), None, None, None, None) == PTX_ERR_ARG
    with pytest.raises(ValueError):
        g.render_temporal(16, 8, 16, 4, 0, 1)  # pass_count < 2
    with pytest.raises(ValueError):
        g.render_temporal(16, 8, 16, 4, 0, 4, n_gpus=2)
    g.close()
