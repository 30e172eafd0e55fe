"""ptx_scene_set_camera_projection / ptx_scene_camera_projection without a GPU: the symbols, the getter's values, a fresh scene's
state, every refusal with its message -- the lens and the projection exclude each other in both orders, and the entry points whose
camera is a pinhole's refuse a lat-long scene before any device is looked at -- and the Python round trip.  A host-only scene
(device -1) is enough: the setter accepts it."""
import ctypes as C

import numpy as np
import pytest

import path_tracer_ocaml_amd as P
from path_tracer_ocaml_amd import abi

PTX_ERR_ARG, PTX_ERR_STATE = -1, -3
WAY_OUT = "ptx_scene_set_camera_projection(scene, PTX_PROJECTION_PERSPECTIVE) first"


@pytest.fixture()
def scene(oracle):
    d = oracle.desc_cornell(16, 8)
    g = P.Scene(d.ptr, -1, keepalive=d)
    yield g
    g.close()


def test_the_symbols_exist():
    L = P.lib()
    for name in ("ptx_scene_set_camera_projection", "ptx_scene_camera_projection"):
        assert name in P.EXPORTS and getattr(L, name)
    assert L.ptx_version() == 6  # only entry points and defines were added
    assert (abi.PTX_PROJECTION_PERSPECTIVE, abi.PTX_PROJECTION_LATLONG) == (0, 1)


def test_a_fresh_scene_is_a_pinhole_and_the_getter_returns_what_was_set(scene):
    L = P.lib()
    assert L.ptx_scene_camera_projection(scene._h) == 0 and scene.camera_projection == "perspective"
    scene.set_camera_projection("latlong")
    assert L.ptx_scene_camera_projection(scene._h) == 1 and scene.camera_projection == "latlong"
    scene.set_camera_projection(abi.PTX_PROJECTION_LATLONG)  # sticky, and setting it again is no error
    assert scene.camera_projection == "latlong"
    scene.set_camera_pose(np.ones(3), np.eye(3))  # the pose and the projection are independent states
    assert scene.camera_projection == "latlong"
    scene.set_camera_pose()
    assert scene.camera_projection == "latlong"
    scene.set_camera_projection("perspective")
    assert L.ptx_scene_camera_projection(scene._h) == 0


@pytest.mark.parametrize("value", [-1, 2, 7])
def test_an_unknown_projection_is_refused(scene, value):
    scene.set_camera_projection("latlong")
    assert P.lib().ptx_scene_set_camera_projection(scene._h, value) == PTX_ERR_ARG
    assert P.last_error().startswith("camera projection: ")
    assert scene.camera_projection == "latlong"  # a refused call changes nothing
    with pytest.raises(ValueError, match="projection must be one of"):
        scene.set_camera_projection("fisheye")


def test_null_scene():
    L = P.lib()
    assert L.ptx_scene_set_camera_projection(None, 1) == PTX_ERR_ARG and "NULL scene" in P.last_error()
    assert L.ptx_scene_camera_projection(None) == PTX_ERR_ARG and "NULL scene" in P.last_error()


def test_the_lens_and_the_projection_exclude_each_other_in_both_orders(scene):
    L = P.lib()
    scene.set_lens(0.05, 3.0)
    assert L.ptx_scene_set_camera_projection(scene._h, 1) == PTX_ERR_STATE
    assert "ptx_scene_set_lens(scene, 0, 1) first" in P.last_error()
    assert scene.camera_projection == "perspective" and scene.lens() == (0.05, 3.0)
    scene.set_camera_projection("perspective")  # the pinhole is never refused
    scene.set_lens(0.0, 3.0)
    scene.set_camera_projection("latlong")
    assert L.ptx_scene_set_lens(scene._h, 0.05, 3.0) == PTX_ERR_STATE
    assert WAY_OUT in P.last_error()
    assert scene.lens() == (0.0, 3.0) and scene.camera_projection == "latlong"
    scene.set_lens(0.0, 1.0)  # radius 0 -- no lens -- is accepted under LATLONG
    with pytest.raises(P.PtxError, match="lat-long projection has no lens"):
        scene.set_lens(0.1, 1.0)


def test_the_pinhole_only_entry_points_refuse_a_panorama_before_any_device(scene, oracle):
    """PTX_ERR_STATE with the way out in the message; a host-only scene gets it too (a pinhole one gets the host-only refusal)"""
    L = P.lib()
    ip, dp = abi.c_int32_p, abi.c_double_p
    xs = np.zeros(4, dtype=np.int32)
    p = P.render_params(16, 8, 4, 4)
    ray, attn, alive = np.zeros((4, 6)), np.zeros((4, 3)), np.zeros(4, dtype=np.int32)
    L.ptx_debug_first_scatter.argtypes = [C.c_void_p, C.POINTER(abi.RenderParams), C.c_int64, ip, ip, ip, dp, dp, ip]
    args = (scene._h, C.byref(p), 4, xs.ctypes.data_as(ip), xs.ctypes.data_as(ip), xs.ctypes.data_as(ip), ray.ctypes.data_as(dp),
            attn.ctypes.data_as(dp), alive.ctypes.data_as(ip))
    lights = oracle.lights_cornell(16, 8)
    ppm = abi.ppm_params(16, 8, iterations=1, photon_count=2000)
    for kind, words in (("latlong", WAY_OUT), ("perspective", "host-only")):
        scene.set_camera_projection(kind)
        assert L.ptx_debug_first_scatter(*args) == PTX_ERR_STATE and words in P.last_error(), P.last_error()
        with pytest.raises(P.PtxError) as e:
            scene.ppm_render(ppm, lights)
        assert "(-3)" in str(e.value) and words in str(e.value)
        with pytest.raises(P.PtxError) as e:
            scene.render_temporal(16, 8, 4, 4, 0, 4)
        assert "(-3)" in str(e.value) and words in str(e.value)


def test_integrator_create_sets_the_projection(oracle):
    from path_tracer_ocaml_amd.integrator import Integrator
    d = oracle.desc_shirley(16, 8)
    g = P.Scene(d.ptr, -1, keepalive=d)
    Integrator.create(width=16, height=8, image=np.zeros((8, 16, 3)), samples_per_pixel=1, max_bounces=2, scene=g, projection="latlong")
    assert g.camera_projection == "latlong"
    g.close()
