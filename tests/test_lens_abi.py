"""ptx_scene_set_lens / ptx_scene_lens without a GPU: the symbols, the getter, every refusal with its message, a fresh scene's state,
the Python round trip.  A host-only scene (device -1) is enough: the setter accepts it, like the film's and the lighting mode's."""
import ctypes as C
import math

import pytest

import path_tracer_ocaml_amd as P

PTX_ERR_ARG = -1


@pytest.fixture(scope="module")
def scene(oracle):
    d = oracle.desc_shirley(16, 8)
    g = P.Scene(d.ptr, -1, keepalive=d)
    yield g
    g.close()


def test_the_symbols_exist():
    L = P.lib()
    assert "ptx_scene_set_lens" in P.EXPORTS and "ptx_scene_lens" in P.EXPORTS
    assert L.ptx_scene_set_lens and L.ptx_scene_lens
    assert L.ptx_version() == 6  # only entry points were added


def test_a_fresh_scene_has_no_lens(oracle):
    d = oracle.desc_shirley(16, 8)
    g = P.Scene(d.ptr, -1, keepalive=d)
    assert g.lens() == (0.0, 1.0)
    g.close()


def test_the_getter_returns_what_was_set(scene):
    L = P.lib()
    for radius, focus in ((0.05, 10.0), (2.0 ** -30, 1e9), (0.0, 3.5), (0.125, 0.5)):
        scene.set_lens(radius, focus)
        assert scene.lens() == (radius, focus)
        r, f = C.c_double(-1.0), C.c_double(-1.0)
        assert L.ptx_scene_lens(scene._h, C.byref(r), None) == 0 and r.value == radius
        assert L.ptx_scene_lens(scene._h, None, C.byref(f)) == 0 and f.value == focus
    scene.set_lens(0.0, 1.0)


@pytest.mark.parametrize("radius, focus, words", [
    (-0.5, 1.0, "radius must be finite and >= 0"), (math.nan, 1.0, "radius must be finite and >= 0"),
    (math.inf, 1.0, "radius must be finite and >= 0"), (-0.0 - 1e-300, 1.0, "radius must be finite and >= 0"),
    (0.1, 0.0, "focus_distance must be finite and > 0"), (0.1, -2.0, "focus_distance must be finite and > 0"),
    (0.1, math.nan, "focus_distance must be finite and > 0"), (0.1, math.inf, "focus_distance must be finite and > 0"),
    (0.0, 0.0, "focus_distance must be finite and > 0")])
def test_refusals_name_the_rule(scene, radius, focus, words):
    scene.set_lens(0.25, 4.0)
    assert P.lib().ptx_scene_set_lens(scene._h, radius, focus) == PTX_ERR_ARG
    msg = P.last_error()
    assert msg.startswith("lens: ") and words in msg, msg
    assert scene.lens() == (0.25, 4.0)  # a refused call changes nothing
    with pytest.raises(P.PtxError, match="lens: "):
        scene.set_lens(radius, focus)
    scene.set_lens(0.0, 1.0)


def test_null_scene():
    L = P.lib()
    assert L.ptx_scene_set_lens(None, 0.1, 1.0) == PTX_ERR_ARG and "NULL scene" in P.last_error()
    r = C.c_double()
    assert L.ptx_scene_lens(None, C.byref(r), None) == PTX_ERR_ARG and "NULL scene" in P.last_error()


def test_integrator_create_sets_the_lens(oracle):
    import numpy as np
    from path_tracer_ocaml_amd.integrator import Integrator
    d = oracle.desc_shirley(16, 8)
    g = P.Scene(d.ptr, -1, keepalive=d)
    Integrator.create(width=16, height=8, image=np.zeros((8, 16, 3)), samples_per_pixel=1, max_bounces=2, scene=g, lens=(0.05, 13.5))
    assert g.lens() == (0.05, 13.5)
    g.close()


@pytest.mark.parametrize("flags, words", [
    (["--lens-radius=-1"], "--lens-radius, must be >= 0"), (["--lens-radius=x"], "--lens-radius, must be >= 0"),
    (["--lens-radius=0.1", "--focus-distance=0"], "--focus-distance, must be > 0"),
    (["--focus-distance=3"], "--focus-distance requires --lens-radius > 0")])
def test_cli_refuses_bad_lens_flags(flags, words):
    """checked while the command line is parsed, before any device is touched: Cmdliner's exit code 124"""
    import os
    import subprocess
    exe = os.path.join(os.path.dirname(os.path.abspath(P.__file__)), "shirley_spheres")
    r = subprocess.run([exe, "-d", "16,8", "--no-progress", *flags], capture_output=True, text=True)
    assert r.returncode == 124 and words in r.stderr, r.stderr


def test_host_scenes_know_their_focus_distance():
    from path_tracer_ocaml_amd import host
    assert host.cornell_box(16, 8, 12.0).focus_distance == 1.0  # eye (0.5, 0.5, -1) -> target (0.5, 0.5, 0)
    assert abs(host.shirley_spheres(16, 8).focus_distance - (13.0 ** 2 + 2.0 ** 2 + 4.5 ** 2) ** 0.5) < 1e-12
