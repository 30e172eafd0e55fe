"""shirley_spheres --turntable=T --temporal[=CAP]: a short sequence over every --scene writes its frames and reports the history
each one took; the flags' refusals are decided while the command line is parsed, before any device is touched."""
import os
import re
import subprocess

import pytest

import path_tracer_ocaml_amd as P

EXE = os.path.join(os.path.dirname(os.path.abspath(P.__file__)), "shirley_spheres")
W, H = 48, 24


@pytest.mark.gpu
@pytest.mark.parametrize("flags", [["--scene=shirley"], ["--scene=cornell", "--denoise"], ["--scene=ganesha", "--triangles=2000", "--temporal=16"]])
def test_a_short_sequence_writes_its_frames_and_keeps_history(tmp_path, flags):
    out = tmp_path / "turn.png"
    cmd = [EXE, "-d", f"{W},{H}", "--no-progress", "--samples-per-pixel=4", "--max-ray-bounces=4", "--turntable=4", "--turntable-arc=3", "-o", str(out)]
    cmd += flags if any(f.startswith("--temporal") for f in flags) else flags + ["--temporal"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    frames = re.findall(r"^frame (\d+) -> (\S+), history = (\d+) pixels$", r.stdout, flags=re.M)
    assert [int(f[0]) for f in frames] == [0, 1, 2, 3], r.stdout
    for k, (_, name, took) in enumerate(frames):
        assert name == str(tmp_path / ("turn-%03d.png" % k)) and os.path.getsize(name) > 0
        # the first frame starts from nothing; three quarters of a degree a frame keeps most of the picture
        assert (int(took) == 0) if k == 0 else (W * H // 2 <= int(took) <= W * H), (k, took)
    assert not out.exists()  # only the numbered frames


@pytest.mark.parametrize("flags, words", [
    (["--temporal"], "--temporal requires --turntable"),
    (["--temporal=8"], "--temporal requires --turntable"),
    (["--turntable=4", "--temporal=-1"], "--temporal, CAP must be >= 0"),
    (["--turntable=4", "--temporal=x"], "--temporal, CAP must be >= 0"),
    (["--turntable=4", "--temporal"], "--temporal requires --samples-per-pixel >= 2"),
    (["--turntable=4", "--temporal", "--samples-per-pixel=4", "--lens-radius=0.1"], "--temporal needs a pinhole"),
    (["--turntable=4", "--temporal", "--samples-per-pixel=4", "--progressive=2"], "--temporal cannot be combined with --adaptive or --progressive"),
    (["--turntable=4", "--temporal", "--samples-per-pixel=4", "--adaptive=0.1"], "--temporal cannot be combined with --adaptive or --progressive"),
    (["--turntable=4", "--temporal", "--samples-per-pixel=4", "--gpus=2"], "--temporal renders on one GPU"),
    (["--turntable=4", "--temporal", "--samples-per-pixel=4", "--denoise", "--aov=x"], "--aov cannot be combined with --temporal"),
    (["--turntable-arc=3"], "--turntable-arc requires --turntable"),
    (["--turntable=4", "--turntable-arc=0"], "--turntable-arc, must be in (0, 360]"),
    (["--turntable=4", "--turntable-arc=361"], "--turntable-arc, must be in (0, 360]"),
    (["--turntable=4", "--turntable-arc=nan"], "--turntable-arc, must be in (0, 360]")])
def test_cli_refuses_bad_temporal_flags(flags, words):
    """Cmdliner's exit code 124, as the other flags' refusals"""
    r = subprocess.run([EXE, "-d", "16,8", "--no-progress", *flags], capture_output=True, text=True)
    assert r.returncode == 124 and words in r.stderr, r.stderr
