"""`shirley_spheres --panorama --hdr-out` on the GPU: the PFM it writes is the binary32 rounding of the square of the image Python's
Scene.render gives under the same state, row for row -- the filmed linear radiance, in the layout --envmap reads back -- and the PNG
is Python's; the flags compose with --camera-eye / --camera-target."""
import os
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H, SPP, DEPTH = 16, 8, 4, 4


@pytest.fixture(scope="module")
def P():
    import path_tracer_ocaml_amd as P
    assert P.lib().ptx_device_count() >= 1, P.last_error()
    return P


def _env():
    env = dict(os.environ)
    env["LD_LIBRARY_PATH"] = "/opt/rocm/lib:" + env.get("LD_LIBRARY_PATH", "")
    return env


def _cli(tmp_path, name, *flags):
    exe = os.path.join(ROOT, "path_tracer_ocaml_amd", "shirley_spheres")
    png, pfm = tmp_path / f"{name}.png", tmp_path / f"{name}.pfm"
    r = subprocess.run([exe, f"--dimension={W},{H}", f"--samples-per-pixel={SPP}", f"--max-ray-bounces={DEPTH}", "--no-progress", "--panorama",
                        f"--hdr-out={pfm}", "-o", str(png), *flags], capture_output=True, text=True, env=_env(), timeout=300)
    assert r.returncode == 0, r.stderr
    return png, pfm


def _same_as_python(P, g, png, pfm, tmp_path):
    from path_tracer_ocaml_amd import host as Hs
    g.set_camera_projection("latlong")
    rgb, _ = g.render(W, H, SPP, DEPTH)
    want = (rgb * rgb).astype(np.float32).astype(np.float64)
    got = Hs.load_pfm(str(pfm))
    assert got.shape == (H, W, 3) and np.array_equal(got.view(np.uint64), want.view(np.uint64))
    assert float(got.max()) > 0.0
    Hs.write_png(str(tmp_path / "py.png"), rgb)
    assert png.read_bytes() == (tmp_path / "py.png").read_bytes()
    return rgb


def test_the_pfm_is_the_square_of_pythons_image_in_binary32(P, tmp_path):
    from path_tracer_ocaml_amd import host as Hs
    png, pfm = _cli(tmp_path, "home")
    hs = Hs.shirley_spheres(W, H)
    g = P.Scene(hs.ptr, 0, keepalive=hs)
    home = _same_as_python(P, g, png, pfm, tmp_path)
    # from another eye: the pose the CLI computes from --camera-eye / --camera-target is camera_pose_look_at's
    eye, target = (9.0, 3.5, -6.0), (0.5, 0.4, 0.3)
    png, pfm = _cli(tmp_path, "moved", "--camera-eye=" + ",".join(map(str, eye)), "--camera-target=" + ",".join(map(str, target)))
    cam = hs.camera
    g.set_camera_pose(*P.camera_pose_look_at(cam["look_at"], eye, target, cam["up"], W / H, cam["fov_deg"]))
    moved = _same_as_python(P, g, png, pfm, tmp_path)
    assert not np.array_equal(moved, home)
    g.close()
