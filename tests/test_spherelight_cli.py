"""shirley_spheres' --light-spheres and --sphere-lamp without a GPU: what the command line refuses, and that the lamp sphere is appended
behind a Shirley scene that is otherwise byte for byte the one without it."""
import os
import subprocess

import numpy as np
import pytest

from path_tracer_ocaml_amd import abi, host

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "path_tracer_ocaml_amd", "shirley_spheres")
LAMP = (0.0, 1.0, 0.0, 1.0, 30.0)  # where the big metal sphere is


@pytest.mark.parametrize("flags, message", [
    (["--light-spheres"], "--light-spheres requires --lighting=sampled"),
    (["--light-spheres", "--lighting=path-order"], "--light-spheres requires --lighting=sampled"),
    (["--sphere-lamp=0,4,0,0.5,30", "--scene=cornell"], "--sphere-lamp requires --scene=shirley"),
    (["--sphere-lamp=0,4,0,0.5"], "invalid value for --sphere-lamp, expected X,Y,Z,R,EMIT"),
    (["--sphere-lamp=0,4,0,0.5,30,1"], "invalid value for --sphere-lamp, expected X,Y,Z,R,EMIT"),
    (["--sphere-lamp=0,4,0,0,30"], "invalid value for --sphere-lamp, R and EMIT must be > 0"),
    (["--sphere-lamp=0,4,0,0.5,-1"], "invalid value for --sphere-lamp, R and EMIT must be > 0"),
    (["--sphere-lamp=0,nan,0,0.5,30"], "invalid value for --sphere-lamp, every number must be finite"),
])
def test_flag_errors(flags, message):
    r = subprocess.run([EXE, "--dimension=8,4", "--no-progress", *flags], capture_output=True, text=True, timeout=60)
    assert r.returncode == 124 and message in r.stderr.split("\n")[0], r.stderr


def _arrays(hs):
    d = hs.ptr.contents
    a = {k: np.ctypeslib.as_array(getattr(d, "sphere_" + k), shape=(d.n_spheres,)).copy() for k in ("x", "y", "z", "r", "material")}
    mats = np.array([[m.kind, m.texture, m.index, *m.emit] for m in (d.materials[i] for i in range(d.n_materials))])
    texs = np.array([[t.kind, t.width, t.height, *t.even, *t.odd] for t in (d.textures[i] for i in range(d.n_textures))])
    return d, a, mats, texs


@pytest.mark.parametrize("no_simd", [False, True])
def test_the_lamp_is_appended_behind_an_unchanged_scene(no_simd):
    hs0, hs1 = host.shirley_spheres(96, 48, no_simd=no_simd), host.shirley_lamp(96, 48, LAMP, no_simd=no_simd)  # (they own the arrays)
    d0, a0, m0, t0 = _arrays(hs0)
    d1, a1, m1, t1 = _arrays(hs1)
    n = d0.n_spheres
    assert d1.n_spheres == n + 1 and d1.n_materials == d0.n_materials + 1 and d1.n_textures == d0.n_textures + 1
    for k in a0:
        assert np.array_equal(a0[k].view(np.uint8), a1[k][:n].view(np.uint8)), k  # no RNG draw moved
    assert np.array_equal(m0, m1[:-1]) and np.array_equal(t0, t1[:-1])
    assert list(m1[-1]) == [abi.PTX_MAT_LAMBERTIAN, d1.n_textures - 1, 0.0, 30.0, 30.0, 30.0]
    assert list(t1[-1][:6]) == [abi.PTX_TEX_SOLID, 0, 0, 1.0, 1.0, 1.0]
    assert a1["material"][-1] == d1.n_materials - 1 and a1["r"][-1] == 1.0
    # world coordinates through the scene's own look-at: the lamp lies where the metal sphere (0, 1, 0) went
    for k in ("x", "y", "z"):
        assert a1[k][-1] == a0[k][2], k
    for f in ("lower_left_x", "lower_left_y", "view_x", "view_y"):
        assert getattr(d0.camera, f) == getattr(d1.camera, f)
    assert (d0.leaf_kind, d0.length_cutoff, d0.num_bins, d0.background.kind) == (d1.leaf_kind, d1.length_cutoff, d1.num_bins, d1.background.kind)
