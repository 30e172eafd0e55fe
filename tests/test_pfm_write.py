"""The hosts' PFM writer (host/pfm.cpp, pth_pfm_write), the mirror of pth_pfm_load: a write / load round trip through the host
library, the refusals, and the stand-alone program tests/c/pfm_write_driver.cpp built with AddressSanitizer +
UndefinedBehaviorSanitizer and run here on the CPU; the command-line flags that use the writer are refused where they cannot be
honoured, while the command line is parsed."""
import os
import subprocess

import numpy as np
import pytest

import path_tracer_ocaml_amd as P
from path_tracer_ocaml_amd import host
from test_sanitizers import built, run_clean  # noqa: F401  (built: the `make asan` fixture)


def _image(h, w, seed):
    rng = np.random.default_rng(seed)
    img = rng.random((h, w, 3)) * 10.0 ** rng.integers(-44, 30, (h, w, 3))
    img[0, 0] = (0.0, -0.0, 1.0 + 2.0 ** -24)  # zeros keep their sign; a tie rounds to even
    return img * rng.choice([-1.0, 1.0], (h, w, 3))


@pytest.mark.parametrize("h, w", [(1, 1), (8, 16), (13, 7), (3, 257)])
def test_a_file_written_and_read_back_is_the_binary32_rounding(tmp_path, h, w):
    img = _image(h, w, h * 1000 + w)
    path = str(tmp_path / "out.pfm")
    host.write_pfm(path, img)
    back = host.load_pfm(path)
    want = img.astype(np.float32).astype(np.float64)
    assert back.shape == (h, w, 3)
    assert np.array_equal(back.view(np.uint64), want.view(np.uint64))  # rows in the same order, signs of zeros included
    raw = open(path, "rb").read()
    header = f"PF\n{w} {h}\n-1.0\n".encode()
    assert raw.startswith(header) and len(raw) == len(header) + 12 * w * h
    assert np.array_equal(np.frombuffer(raw[len(header):], dtype="<f4").reshape(h, w, 3), img.astype(np.float32))


def test_refusals(tmp_path):
    path = str(tmp_path / "bad.pfm")
    for img, words in ((np.full((2, 2, 3), np.nan), "not finite"), (np.full((1, 1, 3), 1e39), "pixel (0, 0) is not finite in binary32"),
                       (np.zeros((0, 4, 3)), "width and height must be in")):
        with pytest.raises(IOError, match=words.replace("(", r"\(").replace(")", r"\)")):
            host.write_pfm(path, img)
        assert not os.path.exists(path)
    with pytest.raises(IOError, match="cannot write"):
        host.write_pfm(str(tmp_path / "no" / "dir" / "x.pfm"), np.zeros((1, 1, 3)))


def test_writer_under_the_sanitizers(built, tmp_path):  # noqa: F811
    out = run_clean([os.path.join(built, "pfm_write_driver"), str(tmp_path)])
    lines = out.strip().splitlines()
    assert len(lines) == 20 and all(line.startswith("ok ") for line in lines), out


@pytest.mark.parametrize("flags, words", [
    (["--panorama", "--lens-radius=0.1"], "--panorama has no lens"),
    (["--panorama", "--turntable=2", "--temporal", "--samples-per-pixel=2"], "--temporal needs a pinhole: it cannot be combined with --panorama"),
    (["--hdr-out="], "invalid value for --hdr-out")])
def test_cli_refuses_what_a_panorama_cannot_do(flags, words):
    """checked while the command line is parsed, before any device is touched: Cmdliner's exit code 124"""
    exe = os.path.join(os.path.dirname(os.path.abspath(P.__file__)), "shirley_spheres")
    r = subprocess.run([exe, "-d", "16,8", "--no-progress", *flags], capture_output=True, text=True)
    assert r.returncode == 124 and words in r.stderr, r.stderr
