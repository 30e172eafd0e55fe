"""ptx_scene_set_camera_pose / ptx_scene_camera_pose without a GPU: the symbols, the getter, the NULL combinations, every refusal with
its message, stickiness, a fresh scene's state, the Python round trip, and the two entry points that refuse a posed scene before they
touch a device.  A host-only scene (device -1) is enough: the setter accepts it, like the lens's and the film's."""
import ctypes as C
import math

import numpy as np
import pytest

import path_tracer_ocaml_amd as P
from path_tracer_ocaml_amd import abi

PTX_ERR_ARG, PTX_ERR_STATE = -1, -3
dp = abi.c_double_p
I3 = np.eye(3)


def _dp(a):
    return a.ctypes.data_as(dp)


@pytest.fixture(scope="module")
def scene(oracle):
    d = oracle.desc_shirley(16, 8)
    g = P.Scene(d.ptr, -1, keepalive=d)
    yield g, d
    g.close()


def _rot(angle=0.3):
    c, s = math.cos(angle), math.sin(angle)
    return np.array([[c, 0.0, s], [0.0, 1.0, 0.0], [-s, 0.0, c]])


def test_the_symbols_exist():
    L = P.lib()
    for name in ("ptx_scene_set_camera_pose", "ptx_scene_camera_pose", "ptx_camera_rays"):
        assert name in P.EXPORTS and getattr(L, name)
    assert L.ptx_version() == 6  # only entry points were added


def test_a_fresh_scene_has_no_pose(scene):
    g, d = scene
    assert g.camera_pose is None
    o, r, v = np.full(3, 7.0), np.full(9, 7.0), abi.Camera()
    assert P.lib().ptx_scene_camera_pose(g._h, _dp(o), _dp(r), C.byref(v)) == 0
    cam = d.ptr.contents.camera
    assert (o == 0.0).all() and np.array_equal(r.reshape(3, 3), I3)
    assert (v.lower_left_x, v.lower_left_y, v.view_x, v.view_y) == (cam.lower_left_x, cam.lower_left_y, cam.view_x, cam.view_y)


def test_the_getter_returns_what_was_set_and_the_pose_is_sticky(scene):
    g, d = scene
    cam = d.ptr.contents.camera
    own = (cam.lower_left_x, cam.lower_left_y, cam.view_x, cam.view_y)
    o, R, view = np.array([1.5, -2.0 ** -30, 1e9]), _rot(), (-0.7, -0.4, 1.4, 0.8)
    g.set_camera_pose(o, R, view)
    for _ in range(2):  # asking changes nothing
        go, gR, gv = g.camera_pose
        assert np.array_equal(go, o) and np.array_equal(gR, R) and gv == view
    g.set_camera_pose(o, R)  # no view: the scene's own
    go, gR, gv = g.camera_pose
    assert np.array_equal(go, o) and np.array_equal(gR, R) and gv == own
    g.set_camera_pose(view=view)  # view alone: origin 0 and the identity
    go, gR, gv = g.camera_pose
    assert (go == 0.0).all() and np.array_equal(gR, I3) and gv == view
    g.set_camera_pose(np.zeros(3), I3)  # the identity is ON
    assert g.camera_pose is not None
    # any out pointer may be NULL
    assert P.lib().ptx_scene_camera_pose(g._h, None, None, None) == 1
    g.set_camera_pose()  # all three NULL: off
    assert g.camera_pose is None and P.lib().ptx_scene_camera_pose(g._h, None, None, None) == 0


BAD = [
    ("origin", None, None, "origin and rotation are given together"),
    (None, "rotation", None, "origin and rotation are given together"),
    ("origin", None, "view", "origin and rotation are given together"),
    ((math.nan, 0.0, 0.0), "rotation", None, "origin must be finite"),
    ((0.0, math.inf, 0.0), "rotation", None, "origin must be finite"),
    ("origin", "nan", None, "rotation must be finite"),
    ("origin", "scaled", None, "max |R R^T - I|"),
    ("origin", "sheared", None, "max |R R^T - I|"),
    ("origin", "mirror", None, "det R > 0"),
    ("origin", "rotation", (math.nan, -1.0, 2.0, 2.0), "view must be finite"),
    (None, None, (-1.0, -1.0, math.inf, 2.0), "view must be finite"),
]


@pytest.mark.parametrize("origin, rotation, view, words", BAD)
def test_refusals_name_the_rule(scene, origin, rotation, view, words):
    g, _ = scene
    good_o, good_R = np.array([0.25, 0.5, -4.0]), _rot(1.1)
    g.set_camera_pose(good_o, good_R)
    rots = {"rotation": _rot(), "nan": np.where(I3 == 1.0, math.nan, 0.0), "scaled": _rot() * (1.0 + 1e-8),
            "sheared": _rot() + np.array([[0.0, 1e-8, 0.0]] * 3), "mirror": np.diag([1.0, 1.0, -1.0])}
    o = None if origin is None else np.array([0.1, 0.2, 0.3] if origin == "origin" else origin, dtype=np.float64)
    R = None if rotation is None else np.ascontiguousarray(rots[rotation], dtype=np.float64)
    v = None if view is None else abi.Camera(*((-1.0, -1.0, 2.0, 2.0) if view == "view" else view))
    rc = P.lib().ptx_scene_set_camera_pose(g._h, None if o is None else _dp(o), None if R is None else _dp(R), None if v is None else C.byref(v))
    assert rc == PTX_ERR_ARG
    msg = P.last_error()
    assert msg.startswith("camera pose: ") and words in msg, msg
    go, gR, _ = g.camera_pose  # a refused call changes nothing
    assert np.array_equal(go, good_o) and np.array_equal(gR, good_R)
    g.set_camera_pose()


def test_a_rotation_within_the_bar_is_accepted(scene):
    g, _ = scene
    g.set_camera_pose(np.zeros(3), _rot() * (1.0 + 1e-10))  # max |R R^T - I| about 2e-10 <= 1e-9
    assert g.camera_pose is not None
    g.set_camera_pose()


def test_null_scene():
    L = P.lib()
    o = np.zeros(3)
    assert L.ptx_scene_set_camera_pose(None, None, None, None) == PTX_ERR_ARG and "NULL scene" in P.last_error()
    assert L.ptx_scene_camera_pose(None, _dp(o), None, None) == PTX_ERR_ARG and "NULL scene" in P.last_error()


def test_the_pinhole_only_entry_points_refuse_a_pose_before_any_device(scene, oracle):
    """PTX_ERR_STATE with the pose's message, returned before the scene's device is looked at: a host-only scene gets it too (with
    the pose off it gets the host-only refusal instead)"""
    g, _ = scene
    L = P.lib()
    xs = np.zeros(4, dtype=np.int32)
    ip = abi.c_int32_p
    p = P.render_params(16, 8, 1, 4)
    ray, attn, alive = np.zeros((4, 6)), np.zeros((4, 3)), np.zeros(4, dtype=np.int32)
    L.ptx_debug_first_scatter.argtypes = [C.c_void_p, C.POINTER(abi.RenderParams), C.c_int64, ip, ip, ip, dp, dp, ip]
    args = (g._h, C.byref(p), 4, xs.ctypes.data_as(ip), xs.ctypes.data_as(ip), xs.ctypes.data_as(ip), _dp(ray), _dp(attn), alive.ctypes.data_as(ip))
    lights = oracle.lights_cornell(16, 8)
    g.set_camera_pose(np.zeros(3), I3)
    assert L.ptx_debug_first_scatter(*args) == PTX_ERR_STATE
    assert "ptx_scene_set_camera_pose(scene, NULL, NULL, NULL) first" in P.last_error()
    with pytest.raises(P.PtxError, match=r"ptx_scene_set_camera_pose\(scene, NULL, NULL, NULL\) first"):
        g.ppm_render(abi.ppm_params(16, 8, iterations=1, photon_count=2000), lights)
    g.set_camera_pose()
    assert L.ptx_debug_first_scatter(*args) == PTX_ERR_STATE and "host-only" in P.last_error()
    with pytest.raises(P.PtxError, match="host-only"):
        g.ppm_render(abi.ppm_params(16, 8, iterations=1, photon_count=2000), lights)


def test_integrator_create_sets_the_pose(oracle):
    from path_tracer_ocaml_amd import host
    from path_tracer_ocaml_amd.integrator import Integrator
    hs = host.shirley_spheres(16, 8)
    g = P.Scene(hs.ptr, -1, keepalive=hs)
    cam = hs.camera
    pose = P.camera_pose_look_at(cam["look_at"], (9.0, 3.5, -6.0), (0.5, 0.4, 0.3), cam["up"], 2.0, 28.0)
    Integrator.create(width=16, height=8, image=np.zeros((8, 16, 3)), samples_per_pixel=1, max_bounces=2, scene=g, camera_pose=pose)
    o, R, view = g.camera_pose
    assert np.array_equal(o, pose[0]) and np.array_equal(R, pose[1]) and view == pose[2]
    g.close()


@pytest.mark.parametrize("flags, words", [
    (["--camera-eye=1,2,3"], "--camera-eye and --camera-target are given together"),
    (["--camera-target=1,2,3"], "--camera-eye and --camera-target are given together"),
    (["--camera-eye=1,2", "--camera-target=0,0,0"], "--camera-eye, expected X,Y,Z"),
    (["--camera-eye=1,2,3", "--camera-target=0,0,nan"], "--camera-target, expected X,Y,Z"),
    (["--camera-eye=1,2,3", "--camera-target=1,2,3"], "must differ"),
    (["--camera-fov=30"], "--camera-fov requires"),
    (["--camera-eye=1,2,3", "--camera-target=0,0,0", "--camera-fov=180"], "--camera-fov, must be in (0, 180)"),
    (["--turntable=0"], "--turntable, must be in 1..999"), (["--turntable=x"], "--turntable, must be in 1..999")])
def test_cli_refuses_bad_camera_flags(flags, words):
    """checked while the command line is parsed, before any device is touched: Cmdliner's exit code 124"""
    import os
    import subprocess
    exe = os.path.join(os.path.dirname(os.path.abspath(P.__file__)), "shirley_spheres")
    r = subprocess.run([exe, "-d", "16,8", "--no-progress", *flags], capture_output=True, text=True)
    assert r.returncode == 124 and words in r.stderr, r.stderr
