"""The surface of image textures and the environment, checkable without a GPU: ptx_image as the C compiler lays it out against
the ctypes mirror, the entry points declared, exported and mirrored with no version touched, and every refusal by its message
through a host-only scene (every argument is checked before any device call)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("ptx_scene_set_texture_image", "ptx_scene_set_environment", "ptx_scene_texture_image", "ptx_scene_environment",
       "ptx_texture_eval", "ptx_environment_eval")


@pytest.fixture(scope="module")
def P():
    import path_tracer_ocaml_amd as P
    return P


@pytest.fixture()
def scene(P):
    from path_tracer_ocaml_amd import host
    hs = host.cornell_box(16, 16, 12.0)
    g = P.Scene(hs.ptr, -1, keepalive=hs)
    yield g
    g.close()


def test_ptx_image_layout_matches_c(P, tmp_path):
    abi = P.abi
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "ptx.h"\nint main(void){'
                   'printf("%zu %zu %zu %zu %zu %zu %zu\\n", sizeof(ptx_image), _Alignof(ptx_image), offsetof(ptx_image, width),'
                   'offsetof(ptx_image, height), offsetof(ptx_image, flags), offsetof(ptx_image, reserved), offsetof(ptx_image, rgb));'
                   'return 0;}\n')
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    I = abi.Image
    assert got == [C.sizeof(I), C.alignment(I), I.width.offset, I.height.offset, I.flags.offset, I.reserved.offset, I.rgb.offset]
    assert got == [24, 8, 0, 4, 8, 12, 16]


def test_entry_points_are_declared_exported_and_mirrored(P):
    header = open(os.path.join(ROOT, "include", "ptx.h")).read()
    for name in NEW:
        assert re.search(r"\b%s\(" % name, header), name
        assert name in P.EXPORTS
        getattr(P.lib(), name)
    for macro, value in (("PTX_IMAGE_BILINEAR", 1), ("PTX_IMAGE_REPEAT_U", 2), ("PTX_IMAGE_REPEAT_V", 4), ("PTX_IMAGE_MAX_SIZE", 16384)):
        assert re.search(r"#define %s\s+%d\b" % (macro, value), header), macro
        assert getattr(P.abi, macro) == value
    assert P.lib().ptx_version() == 6  # entry points and one new struct only: no existing struct and no version changed


def _set_tex(P, g, index, arr, flags=0, reserved=0):
    img, keep = P.abi.image(arr, flags)
    img.reserved = reserved
    rc = P.lib().ptx_scene_set_texture_image(g._h, index, C.byref(img))
    return rc, P.last_error()


def _set_env(P, g, arr, flags=0, R=None):
    img, keep = P.abi.image(arr, flags)
    rot = None if R is None else np.ascontiguousarray(R, dtype=np.float64)
    rc = P.lib().ptx_scene_set_environment(g._h, C.byref(img), rot.ctypes.data_as(P.abi.c_double_p) if rot is not None else None)
    return rc, P.last_error()


def test_every_refusal_names_what_was_wrong(P, scene):
    L, g = P.lib(), scene
    ok = np.full((2, 3, 3), 0.5)
    assert L.ptx_scene_set_texture_image(None, 0, None) == -1 and "NULL scene" in P.last_error()
    assert L.ptx_scene_set_environment(None, None, None) == -1 and "NULL scene" in P.last_error()
    # the texture index
    n_tex = g._keep.ptr.contents.n_textures
    for bad in (-1, n_tex, n_tex + 7):
        rc, msg = _set_tex(P, g, bad, ok)
        assert rc == -1 and "texture index %d out of range" % bad in msg and "%d entries" % n_tex in msg
        out = P.abi.Image()
        assert L.ptx_scene_texture_image(g._h, bad, C.byref(out)) == -1 and "out of range" in P.last_error()
    # sizes 0 and 16385 (the array behind them is never read: the size is checked first)
    for w, h in ((0, 2), (2, 0), (16385, 1), (1, 16385), (-1, 1)):
        img = P.abi.Image(w, h, 0, 0, ok.ctypes.data_as(P.abi.c_double_p))
        assert L.ptx_scene_set_texture_image(g._h, 0, C.byref(img)) == -1
        assert "size %d x %d" % (w, h) in P.last_error() and "[1, 16384]" in P.last_error()
        assert L.ptx_scene_set_environment(g._h, C.byref(img), None) == -1
        assert "environment size %d x %d" % (w, h) in P.last_error()
    # flags
    rc, msg = _set_tex(P, g, 0, ok, flags=8)
    assert rc == -1 and "unknown bits in flags (0x8)" in msg
    rc, msg = _set_env(P, g, ok, flags=16 | 1)
    assert rc == -1 and "unknown bits in flags (0x11)" in msg
    for rep in (P.abi.PTX_IMAGE_REPEAT_U, P.abi.PTX_IMAGE_REPEAT_V, 7):
        rc, msg = _set_env(P, g, ok, flags=rep)
        assert rc == -1 and "a repeat flag is not accepted" in msg
    rc, msg = _set_tex(P, g, 0, ok, reserved=1)
    assert rc == -1 and "reserved must be 0" in msg
    img = P.abi.Image(2, 2, 0, 0, None)
    assert L.ptx_scene_set_texture_image(g._h, 0, C.byref(img)) == -1 and "rgb is NULL" in P.last_error()
    # texels
    for bad in (np.nan, np.inf, -np.inf):
        arr = ok.copy()
        arr[1, 2, 1] = bad
        rc, msg = _set_tex(P, g, 0, arr)
        assert rc == -1 and "texel (2, 1) channel 1 is not finite" in msg
        rc, msg = _set_env(P, g, arr)
        assert rc == -1 and "environment: texel (2, 1) channel 1 is not finite" in msg
    # R
    for k in (0, 8):
        R = np.eye(3).reshape(-1)
        R[k] = np.nan
        rc, msg = _set_env(P, g, ok, R=R)
        assert rc == -1 and "R[%d] is not finite" % k in msg
    # nothing that was refused stuck
    assert g.texture_image(0) is None and g.environment() is None
    # the diagnostics refuse a scene without a device, like every compute entry point
    out = np.zeros(3)
    assert L.ptx_texture_eval(g._h, 0, 1, out.ctypes.data_as(P.abi.c_double_p), out.ctypes.data_as(P.abi.c_double_p)) == -3
    assert L.ptx_environment_eval(g._h, 1, out.ctypes.data_as(P.abi.c_double_p), out.ctypes.data_as(P.abi.c_double_p)) == -3
    assert "host-only" in P.last_error()


def test_a_host_only_scene_accepts_valid_calls_and_the_getters_answer(P, scene):
    """as ptx_scene_set_lighting: the state can be set and inspected without a GPU"""
    g = scene
    img = np.random.default_rng(1).uniform(0, 1, (5, 3, 3))
    g.set_texture_image(4, img, bilinear=True, repeat=(True, False))
    assert g.texture_image(4) == (3, 5, P.abi.PTX_IMAGE_BILINEAR | P.abi.PTX_IMAGE_REPEAT_U)
    assert g.texture_image(0) is None
    g.set_texture_image(4, img, repeat=(False, True))
    assert g.texture_image(4) == (3, 5, P.abi.PTX_IMAGE_REPEAT_V)
    g.set_texture_image(4, None)
    assert g.texture_image(4) is None
    g.set_texture_image(0, None)  # restoring what was never set is no error
    R = np.array([[0.0, 0.0, 1.0], [0.0, 1.0, 0.0], [-1.0, 0.0, 0.0]])
    g.set_environment(img, rotation=R)
    (w, h, flags), rot = g.environment()
    assert (w, h, flags) == (3, 5, P.abi.PTX_IMAGE_BILINEAR) and np.array_equal(rot, R)
    g.set_environment(img, bilinear=False)
    (w, h, flags), rot = g.environment()
    assert flags == 0 and np.array_equal(rot, np.eye(3))  # NULL R is the identity
    g.set_environment(None)
    assert g.environment() is None
    with pytest.raises(ValueError):
        g.set_environment(img, rotation=np.eye(2))
    with pytest.raises(ValueError):
        g.set_texture_image(0, np.zeros((4, 4)))


def test_integrator_create_takes_environment_and_images(P):
    from path_tracer_ocaml_amd import host
    from path_tracer_ocaml_amd.integrator import Integrator
    out = np.zeros((16, 16, 3))
    hs = host.cornell_box(16, 16, 12.0)
    env, tex = np.full((4, 8, 3), 0.25), np.full((2, 2, 3), 0.5)
    it = Integrator.create(width=16, height=16, image=out, samples_per_pixel=1, max_bounces=2, scene=hs, device=-1,
                           environment=(env, np.eye(3), False), images={4: (tex, True, (True, True)), 0: tex})
    assert it._scene.environment()[0] == (8, 4, 0)
    assert it._scene.texture_image(4) == (2, 2, 7) and it._scene.texture_image(0) == (2, 2, 0)
    it2 = Integrator.create(width=16, height=16, image=out, samples_per_pixel=1, max_bounces=2, scene=it._scene)  # left as they are
    assert it2._scene.environment()[0] == (8, 4, 0)
    it3 = Integrator.create(width=16, height=16, image=out, samples_per_pixel=1, max_bounces=2, scene=it._scene, environment=env)
    assert it3._scene.environment()[0] == (8, 4, 1)
