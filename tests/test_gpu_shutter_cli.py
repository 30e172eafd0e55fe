"""`shirley_spheres --shutter / --shutter-eye` on the GPU, at 32 x 16 and spp 4: `--turntable=3 --shutter=0.5` writes three files, each
the PNG of Python's image of the same state (frame f's pose, and a shutter half of the way to frame f + 1's); `--shutter-eye` exposes
one frame between two poses; `--shutter` with `--temporal` exits 124 with the library's message; and without the flags the files are
byte for byte what the commit before the shutter wrote (their SHA-256, recorded from that commit's binaries on the MI355X)."""
import hashlib
import os
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H, SPP = 32, 16, 4
# sha256 of the files the parent commit's shirley_spheres writes for `-d 32,16 --samples-per-pixel=4 --no-progress`: the plain render,
# and the three frames of --turntable=3
PARENT = {
    "plain": "e9a97e71b7a3d3ede706fe9bad11f355732bedb5d5193482acb48879cb288f41",
    "turn-000": "e9a97e71b7a3d3ede706fe9bad11f355732bedb5d5193482acb48879cb288f41",
    "turn-001": "d94d45dc5f5c8f06d292c243625e24883084a4b20e1fa826abe694e8c2fa8da2",
    "turn-002": "f287136097aac1bceb821e6a2ff993735f7a4de85d556f27fd29410c2114b8ba",
}


@pytest.fixture(scope="module")
def P():
    import path_tracer_ocaml_amd as P
    assert P.lib().ptx_device_count() >= 1, P.last_error()
    return P


def _run(*flags):
    env = dict(os.environ)
    env["LD_LIBRARY_PATH"] = "/opt/rocm/lib:" + env.get("LD_LIBRARY_PATH", "")
    exe = os.path.join(ROOT, "path_tracer_ocaml_amd", "shirley_spheres")
    return subprocess.run([exe, f"--dimension={W},{H}", f"--samples-per-pixel={SPP}", "--no-progress", *flags], capture_output=True, text=True,
                          env=env, timeout=300)


def _turntable_pose(P, cam, frame, n):
    """render_command.cpp's camera_of_frame, operation for operation (the same libm)"""
    import math
    eye, target, up = ([float(v) for v in cam[k]] for k in ("eye", "target", "up"))
    ln = math.sqrt(up[0] * up[0] + up[1] * up[1] + up[2] * up[2])
    k = [u / ln for u in up]
    th = 2.0 * 3.14159265358979323846 * float(frame) / float(n)
    c, s = math.cos(th), math.sin(th)
    v = [eye[i] - target[i] for i in range(3)]
    kxv = [k[1] * v[2] - k[2] * v[1], k[2] * v[0] - k[0] * v[2], k[0] * v[1] - k[1] * v[0]]
    kv = k[0] * v[0] + k[1] * v[1] + k[2] * v[2]
    eye = [target[i] + (v[i] * c + kxv[i] * s + k[i] * kv * (1.0 - c)) for i in range(3)]
    return P.camera_pose_look_at(cam["look_at"], eye, target, cam["up"], W / H, cam["fov_deg"])


def test_turntable_frames_under_a_shutter_are_pythons_images(P, tmp_path):
    from path_tracer_ocaml_amd import host
    n, fraction = 3, 0.5
    r = _run(f"--turntable={n}", f"--shutter={fraction}", "-o", str(tmp_path / "blur.png"))
    assert r.returncode == 0, r.stderr
    hs = host.shirley_spheres(W, H)
    g = P.Scene(hs.ptr, 0, keepalive=hs)
    frames = []
    for f in range(n):
        pose, nxt = _turntable_pose(P, hs.camera, f, n), _turntable_pose(P, hs.camera, f + 1, n)
        T, k, A = P.camera_shutter_between(pose[0], pose[1], nxt[0], nxt[1])
        assert A > 1.0  # a third of a turn between frames
        g.set_camera_pose(*pose)
        still, _ = g.render(W, H, SPP, 8)
        g.set_camera_shutter(T * fraction, k, A * fraction)
        want, _ = g.render(W, H, SPP, 8)
        assert not np.array_equal(want, still)
        host.write_png(str(tmp_path / "want.png"), want)
        frames.append((tmp_path / f"blur-{f:03d}.png").read_bytes())
        assert frames[f] == (tmp_path / "want.png").read_bytes(), f
        g.set_camera_shutter(None)
    assert len(set(frames)) == n and not (tmp_path / "blur.png").exists()
    g.close()


def test_a_single_frame_between_two_eyes_is_pythons_image(P, tmp_path):
    from path_tracer_ocaml_amd import host
    eye, target, eye1, target1 = (9.0, 3.5, -6.0), (0.5, 0.4, 0.3), (9.5, 3.0, -5.0), (0.4, 0.4, 0.5)
    fmt = lambda v: ",".join(map(str, v))  # noqa: E731
    hs = host.shirley_spheres(W, H)
    cam = hs.camera
    g = P.Scene(hs.ptr, 0, keepalive=hs)
    pose = P.camera_pose_look_at(cam["look_at"], eye, target, cam["up"], W / H, cam["fov_deg"])
    g.set_camera_pose(*pose)
    for flags, end in (([f"--shutter-eye={fmt(eye1)}", f"--shutter-target={fmt(target1)}"], (eye1, target1)), ([f"--shutter-eye={fmt(eye1)}"], (eye1, target))):
        r = _run(f"--camera-eye={fmt(eye)}", f"--camera-target={fmt(target)}", *flags, "-o", str(tmp_path / "got.png"))
        assert r.returncode == 0, r.stderr
        nxt = P.camera_pose_look_at(cam["look_at"], end[0], end[1], cam["up"], W / H, cam["fov_deg"])
        g.set_camera_shutter(*P.camera_shutter_between(pose[0], pose[1], nxt[0], nxt[1]))
        want, _ = g.render(W, H, SPP, 8)
        host.write_png(str(tmp_path / "want.png"), want)
        assert (tmp_path / "got.png").read_bytes() == (tmp_path / "want.png").read_bytes(), flags
    g.close()


def test_a_shutter_under_temporal_exits_124_with_the_librarys_message(tmp_path):
    r = _run("--turntable=3", "--shutter=0.5", "--temporal", "-o", str(tmp_path / "t.png"))
    assert r.returncode == 124, (r.returncode, r.stderr)
    assert "ptx_render_temporal: temporal rendering takes one pose per frame" in r.stderr
    assert "ptx_scene_set_camera_shutter(scene, NULL, NULL, 0) first" in r.stderr
    assert not list(tmp_path.iterdir())


def test_without_the_flags_every_file_is_what_it_was(tmp_path):
    r = _run("-o", str(tmp_path / "plain.png"))
    assert r.returncode == 0, r.stderr
    r = _run("--turntable=3", "-o", str(tmp_path / "turn.png"))
    assert r.returncode == 0, r.stderr
    got = {name: hashlib.sha256((tmp_path / f"{name}.png").read_bytes()).hexdigest() for name in PARENT}
    assert got == PARENT
