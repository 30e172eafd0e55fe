"""The density builder of environment sampling (csrc/scene_host.cpp: scene_env_density, scene_check_env_rotation) under ASan + UBSan,
through the stand-alone driver tests/c/env_density_driver.cpp (`make asan`): every run exits 0 with nothing from the sanitizers on
stderr, and the table it writes is the numpy restatement's bit for bit."""
import os

import numpy as np
import pytest

import envlight_reference as E
import envlight_support as S
from test_sanitizers import ENV, ROOT, built, run_clean  # noqa: F401  (built: the `make asan` fixture)

IMAGES = dict(S.table_images())
IMAGES["sun 300x150"] = S.sun_sky(300, 150, sun=(200, 100))
IMAGES["all zero"] = np.zeros((3, 4, 3))


@pytest.mark.parametrize("name", list(IMAGES))
def test_density_builder_under_sanitizers(built, oracle, tmp_path, name):
    img = np.ascontiguousarray(IMAGES[name], dtype=np.float64)
    H, W = img.shape[:2]
    src, out = str(tmp_path / "rgb.bin"), str(tmp_path / "table.bin")
    img.tofile(src)
    text = run_clean([os.path.join(built, "env_density_driver"), "density", str(W), str(H), src, out])
    head = text.split("\n")[0].split()
    rc, total, last_row, n = int(head[1]), float.fromhex(head[3]), int(head[5]), int(head[7])
    den = E.density(img)
    assert n == 2 + 2 * H + 2 * W * H and total == den.T and last_row == den.last_row
    assert rc == (0 if den.T > 0.0 else -1)
    if rc:
        assert "total weight" in text
    t = np.fromfile(out)
    assert t[0] == den.T and t[1] == den.last_row
    t = t[2:]  # T, last row, then m[H], last column [H], c[H x W], w[H x W]
    assert np.array_equal(S.bits(t[:H]), S.bits(den.m))
    assert np.array_equal(t[H:2 * H].astype(np.int64), den.last_col)
    assert np.array_equal(S.bits(t[2 * H:2 * H + W * H]), S.bits(den.c.ravel()))
    assert np.array_equal(S.bits(t[2 * H + W * H:]), S.bits(den.w.ravel()))


@pytest.mark.parametrize("R, ok", [(np.eye(3), True), (S.rotation([0.3, 1.0, 0.2], 50.0), True), (np.eye(3) * (1.0 + 1e-8), False),
                                  (np.zeros((3, 3)), False), (np.full((3, 3), np.nan), False)])
def test_rotation_check_under_sanitizers(built, R, ok):
    text = run_clean([os.path.join(built, "env_density_driver"), "rotation", *[repr(float(x)) for x in np.asarray(R).ravel()]])
    assert text.split("\n")[0] == ("rc 0" if ok else "rc -1")
    if not ok:
        assert "R R^T" in text
