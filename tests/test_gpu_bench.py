"""bench.py on the GPU: a plain run's line, and `--dump-outputs`, whose arrays are the
framebuffer of the last timed step (whole, or a fixed sample of a frame larger than the limit)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(*flags, timeout=600):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", *flags], capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [json.loads(l) for l in r.stdout.splitlines() if l.startswith("{") and l.rstrip().endswith("}")]
    assert len(lines) == 1, r.stdout[-2000:]
    return lines[0]


def test_plain_run_dumps_the_timed_frame(oracle, tmp_path):
    w, h, spp, depth = 600, 300, 32, 8
    out = tmp_path / "out"
    line = _run("--steps", "3", "--warmup", "1", "--workload", "shirley_600x300_spp32_d8", "--dump-outputs", str(out))
    assert line["steps"] == 3 and line["warmup"] == 1 and line["value"] > 0 and line["ms_per_step"] > 0
    assert abs(line["value"] - w * h * spp / line["ms_per_step"] * 1e-3) <= 1e-9 * line["value"]
    assert not set(line) & {"cpu_baseline", "parity", "roofline", "workloads"}
    assert line["outputs"]["arrays"] == {"rgb": [h, w, 3]}
    assert sorted(os.listdir(out)) == ["rgb.npy"]
    rgb = np.load(out / "rgb.npy")
    assert rgb.dtype == np.float64 and rgb.shape == (h, w, 3)
    d = oracle.desc_shirley(w, h)
    ref = oracle.Scene(d.ptr, d).render(w, h, spp, depth, threads=8)["rgb"]
    assert float((np.abs(rgb - ref) / np.maximum(np.abs(ref), 1e-3)).max()) <= 1e-5


def test_dump_of_a_large_frame_is_a_fixed_sample(tmp_path):
    """The 4K frame (199 MB in binary64) is over the 64 MB limit: the same seeded sample of whole pixels in every run."""
    dirs = [tmp_path / "a", tmp_path / "b"]
    for d in dirs:
        line = _run("--steps", "1", "--warmup", "0", "--workload", "shirley_4k_spp256_d8", "--dump-outputs", str(d))
        assert line["outputs"]["arrays"] == {"rgb_sample": [1 << 20, 3], "rgb_sample_pixel": [1 << 20]}
    got = [{n: np.load(d / (n + ".npy")) for n in ("rgb_sample", "rgb_sample_pixel")} for d in dirs]
    assert sum(a.nbytes for a in got[0].values()) <= 64 << 20
    pix = got[0]["rgb_sample_pixel"]
    assert pix.dtype == np.float64 and np.all(np.diff(pix) > 0) and pix[0] >= 0 and pix[-1] < 3840 * 2160
    assert np.isfinite(got[0]["rgb_sample"]).all() and got[0]["rgb_sample"].max() > 0.5
    for n in got[0]:
        assert np.array_equal(got[0][n], got[1][n]), n
