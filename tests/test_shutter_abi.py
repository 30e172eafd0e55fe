"""ptx_scene_set_camera_shutter / ptx_scene_camera_shutter without a GPU: the symbols, the getter, the NULL combinations, every refusal
with its message, stickiness, a fresh scene's state, the Python round trip, the entry points that refuse a shutter scene before they
touch a device, and the depth a lens and a shutter leave the sampler.  A host-only scene (device -1) is enough: the setter accepts
it, like the pose's."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

import path_tracer_ocaml_amd as P
from path_tracer_ocaml_amd import abi, host

PTX_ERR_ARG, PTX_ERR_STATE = -1, -3
dp, ip = abi.c_double_p, abi.c_int32_p
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WAY_OUT = "ptx_scene_set_camera_shutter(scene, NULL, NULL, 0) first"
T0, K0, A0 = np.array([0.25, -2.0 ** -30, 1e9]), np.array([0.6, 0.0, -0.8]), -0.75


def _dp(a):
    return None if a is None else a.ctypes.data_as(dp)


@pytest.fixture(scope="module")
def scene(oracle):
    d = oracle.desc_shirley(16, 8)
    g = P.Scene(d.ptr, -1, keepalive=d)
    yield g
    g.close()


def test_the_symbols_are_declared_exported_and_mirrored():
    L = P.lib()
    header = open(os.path.join(ROOT, "include", "ptx.h")).read()
    for name in ("ptx_scene_set_camera_shutter", "ptx_scene_camera_shutter"):
        assert name in P.EXPORTS and getattr(L, name)
        assert re.search(r"^int32_t %s\(" % name, header, re.M), name
    assert L.ptx_scene_set_camera_shutter.argtypes == [C.c_void_p, dp, dp, C.c_double]
    assert L.ptx_scene_camera_shutter.argtypes == [C.c_void_p, dp, dp, dp]
    assert L.ptx_version() == 6  # only entry points were added
    assert "pth_camera_shutter_between" in host.EXPORTS and host.lib().pth_camera_shutter_between
    # both "out of scope" sentences are gone from the header
    assert "Out of scope: shutter motion blur" not in header and "focus by picking a pixel, motion blur" not in header


def test_a_fresh_scene_has_no_shutter(scene):
    assert scene.camera_shutter is None
    t, k, a = np.full(3, 7.0), np.full(3, 7.0), C.c_double(7.0)
    assert P.lib().ptx_scene_camera_shutter(scene._h, _dp(t), _dp(k), C.cast(C.byref(a), dp)) == 0
    assert (t == 0.0).all() and (k == 0.0).all() and a.value == 0.0


def test_the_getter_returns_what_was_set_and_the_shutter_is_sticky(scene):
    L = P.lib()
    scene.set_camera_shutter(T0, K0, A0)
    for _ in range(2):  # asking changes nothing
        t, k, a = scene.camera_shutter
        assert np.array_equal(t, T0) and np.array_equal(k, K0) and a == A0
    scene.set_camera_pose(np.ones(3), np.eye(3))  # the pose, the lens and the shutter are independent states
    scene.set_lens(0.1, 3.0)
    t, k, a = scene.camera_shutter
    assert np.array_equal(t, T0) and np.array_equal(k, K0) and a == A0
    scene.set_lens(0.0, 1.0)
    scene.set_camera_pose()
    assert scene.camera_shutter is not None
    assert L.ptx_scene_camera_shutter(scene._h, None, None, None) == 1  # any out pointer may be NULL
    z = np.zeros(3)
    scene.set_camera_shutter(z, z, 0.0)  # no motion, a zero axis: ON
    t, k, a = scene.camera_shutter
    assert (t == 0.0).all() and (k == 0.0).all() and a == 0.0
    scene.set_camera_shutter(T0, np.array([0.0, 3.0, 0.0]), 0.0)  # the axis is not looked at while the angle is 0
    assert scene.camera_shutter is not None
    scene.set_camera_shutter(z, K0, math.pi)  # |angle| = pi is accepted
    assert scene.camera_shutter[2] == math.pi
    scene.set_camera_shutter(z, K0 * (1.0 + 5e-10), -math.pi)  # | |axis| - 1 | = 5e-10 <= 1e-9
    scene.set_camera_shutter()  # NULL, NULL, 0: off
    assert scene.camera_shutter is None and L.ptx_scene_camera_shutter(scene._h, None, None, None) == 0
    scene.set_camera_shutter(T0, K0, A0)
    scene.set_camera_shutter(None)  # Python's other spelling of off
    assert scene.camera_shutter is None


NAN, INF = math.nan, math.inf
BAD = [
    ("T", None, 0.0, "translation and axis are given together"),
    (None, "k", 0.0, "translation and axis are given together"),
    ("T", None, 0.5, "translation and axis are given together"),
    (None, None, 0.5, "translation and axis are given together"),
    ((NAN, 0.0, 0.0), "k", 0.1, "translation must be finite"),
    ((0.0, -INF, 0.0), "k", 0.1, "translation must be finite"),
    ("T", (0.0, NAN, 1.0), 0.1, "axis must be finite"),
    ("T", (INF, 0.0, 0.0), 0.0, "axis must be finite"),
    ("T", "k", NAN, "angle must be finite"),
    ("T", "k", INF, "angle must be finite"),
    (None, None, NAN, "angle must be finite"),
    ("T", "k", 3.1416, "|angle| must be at most pi"),
    ("T", "k", -4.0, "|angle| must be at most pi"),
    ("T", (0.6, 0.0, -0.8 * (1.0 + 1e-8)), 0.1, "| |axis| - 1 |"),
    ("T", (0.0, 0.0, 0.0), 1e-300, "| |axis| - 1 |"),
    ("T", (0.0, 2.0, 0.0), -0.1, "| |axis| - 1 |"),
]


@pytest.mark.parametrize("translation, axis, angle, words", BAD)
def test_refusals_name_the_rule(scene, translation, axis, angle, words):
    scene.set_camera_shutter(T0, K0, A0)
    t = None if translation is None else np.array([0.1, 0.2, 0.3] if translation == "T" else translation, dtype=np.float64)
    k = None if axis is None else np.array([0.0, 1.0, 0.0] if axis == "k" else axis, dtype=np.float64)
    assert P.lib().ptx_scene_set_camera_shutter(scene._h, _dp(t), _dp(k), angle) == PTX_ERR_ARG
    msg = P.last_error()
    assert msg.startswith("camera shutter: ") and words in msg, msg
    gt, gk, ga = scene.camera_shutter  # a refused call changes nothing
    assert np.array_equal(gt, T0) and np.array_equal(gk, K0) and ga == A0
    scene.set_camera_shutter()


def test_null_scene():
    L = P.lib()
    t = np.zeros(3)
    assert L.ptx_scene_set_camera_shutter(None, None, None, 0.0) == PTX_ERR_ARG and "NULL scene" in P.last_error()
    assert L.ptx_scene_camera_shutter(None, _dp(t), None, None) == PTX_ERR_ARG and "NULL scene" in P.last_error()


def test_the_entry_points_without_a_shutter_refuse_it_before_any_device(scene, oracle):
    """PTX_ERR_STATE with the way out in the message, returned before the scene's device is looked at: a host-only scene gets it too
    (with the shutter off it gets the host-only refusal instead); the outputs are not touched"""
    L = P.lib()
    xs = np.zeros(4, dtype=np.int32)
    p = P.render_params(16, 8, 4, 4)
    ray, attn, alive = np.full((4, 6), 7.0), np.full((4, 3), 7.0), np.full(4, 7, dtype=np.int32)
    L.ptx_debug_first_scatter.argtypes = [C.c_void_p, C.POINTER(abi.RenderParams), C.c_int64, ip, ip, ip, dp, dp, ip]
    args = (scene._h, C.byref(p), 4, xs.ctypes.data_as(ip), xs.ctypes.data_as(ip), xs.ctypes.data_as(ip), _dp(ray), _dp(attn), alive.ctypes.data_as(ip))
    lights = oracle.lights_cornell(16, 8)
    ppm = abi.ppm_params(16, 8, iterations=1, photon_count=2000)
    for shutter, words in (((np.zeros(3), np.zeros(3), 0.0), WAY_OUT), ((None, None, 0.0), "host-only")):
        scene.set_camera_shutter(*shutter)
        assert L.ptx_debug_first_scatter(*args) == PTX_ERR_STATE and words in P.last_error(), P.last_error()
        assert (ray == 7.0).all() and (attn == 7.0).all() and (alive == 7).all()
        with pytest.raises(P.PtxError) as e:
            scene.ppm_render(ppm, lights)
        assert "(-3)" in str(e.value) and words in str(e.value)
        with pytest.raises(P.PtxError) as e:
            scene.render_temporal(16, 8, 4, 4, 0, 4)
        assert "(-3)" in str(e.value) and words in str(e.value)


def test_a_lens_and_a_shutter_leave_125_bounces(scene):
    """d = 2 + 2 * max_bounces + 2 + 1 must stay <= 256: 126 is refused (before the device is looked at), 125 is not; without a lens,
    or without a shutter, 126 stays legal"""
    L = P.lib()
    xs = np.zeros(1, dtype=np.int32)
    o, d = np.full(3, 7.0), np.full(3, 7.0)

    def rays(depth):
        p = P.render_params(16, 8, 1, depth)
        rc = L.ptx_camera_rays(scene._h, C.byref(p), 1, xs.ctypes.data_as(ip), xs.ctypes.data_as(ip), xs.ctypes.data_as(ip), _dp(o), _dp(d))
        return rc, P.last_error()
    scene.set_camera_shutter(T0, K0, A0)
    scene.set_lens(0.1, 3.0)
    rc, msg = rays(126)
    assert rc == PTX_ERR_ARG and msg.startswith("camera shutter: ") and "at most 125 bounces with a lens" in msg, msg
    with pytest.raises(P.PtxError, match="at most 125 bounces with a lens"):
        scene.render(16, 8, 1, 126)
    rc, msg = rays(125)
    assert rc == PTX_ERR_STATE and "host-only" in msg, msg  # accepted as far as a host-only scene goes
    rc, msg = rays(127)
    assert rc == PTX_ERR_STATE and "host-only" in msg, msg  # (past 126: the params' own refusal, after the device's)
    scene.set_lens(0.0, 1.0)
    rc, msg = rays(126)
    assert rc == PTX_ERR_STATE and "host-only" in msg, msg
    scene.set_lens(0.1, 3.0)
    scene.set_camera_shutter()
    rc, msg = rays(126)
    assert rc == PTX_ERR_STATE and "host-only" in msg, msg
    scene.set_lens(0.0, 1.0)
    assert (o == 7.0).all() and (d == 7.0).all()


def test_integrator_create_sets_the_shutter_between_two_poses(oracle):
    from path_tracer_ocaml_amd.integrator import Integrator
    hs = host.shirley_spheres(16, 8)
    g = P.Scene(hs.ptr, -1, keepalive=hs)
    cam = hs.camera
    pose0 = P.camera_pose_look_at(cam["look_at"], (9.0, 3.5, -6.0), (0.5, 0.4, 0.3), cam["up"], 2.0, 28.0)
    pose1 = P.camera_pose_look_at(cam["look_at"], (9.5, 3.0, -5.0), (0.4, 0.4, 0.5), cam["up"], 2.0, 28.0)
    shutter = P.camera_shutter_between(pose0[0], pose0[1], pose1[0], pose1[1])
    assert 0.0 < shutter[2] < 0.5 and abs(np.linalg.norm(shutter[1]) - 1.0) <= 1e-9
    Integrator.create(width=16, height=8, image=np.zeros((8, 16, 3)), samples_per_pixel=1, max_bounces=2, scene=g, camera_pose=pose0,
                      camera_shutter=shutter)
    t, k, a = g.camera_shutter
    assert np.array_equal(t, shutter[0]) and np.array_equal(k, shutter[1]) and a == shutter[2]
    assert np.array_equal(g.camera_pose[0], pose0[0])
    g.close()


@pytest.mark.parametrize("flags, words", [
    (["--shutter=0.5"], "--shutter requires --turntable"),
    (["--turntable=3", "--shutter=0"], "--shutter, must be in (0, 1]"),
    (["--turntable=3", "--shutter=1.5"], "--shutter, must be in (0, 1]"),
    (["--turntable=3", "--shutter=x"], "--shutter, must be in (0, 1]"),
    (["--shutter-eye=1,2,3"], "--shutter-eye requires --camera-eye"),
    (["--turntable=3", "--camera-eye=1,2,3", "--camera-target=0,0,0", "--shutter-eye=1,2,4"], "--shutter-eye requires --camera-eye"),
    (["--camera-eye=1,2,3", "--camera-target=0,0,0", "--shutter-eye=1,2"], "--shutter-eye, expected X,Y,Z"),
    (["--camera-eye=1,2,3", "--camera-target=0,0,0", "--shutter-target=1,2,3"], "--shutter-target requires --shutter-eye"),
    (["--camera-eye=1,2,3", "--camera-target=0,0,0", "--shutter-eye=0,0,0"], "--shutter-eye and its target must differ")])
def test_cli_refuses_bad_shutter_flags(flags, words):
    """checked while the command line is parsed, before any device is touched: Cmdliner's exit code 124"""
    import subprocess
    exe = os.path.join(os.path.dirname(os.path.abspath(P.__file__)), "shirley_spheres")
    r = subprocess.run([exe, "-d", "16,8", "--no-progress", *flags], capture_output=True, text=True)
    assert r.returncode == 124 and words in r.stderr, r.stderr
