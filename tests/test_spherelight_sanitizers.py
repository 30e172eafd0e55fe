"""The sphere light list and table (csrc/scene_host.cpp: the emissive-sphere list of scene_set_tree, sphere_light_table_build) under
ASan + UBSan, through the stand-alone driver tests/c/sphere_light_driver.cpp (`make asan`): every run exits 0 with nothing from the
sanitizers on stderr, and the table it writes is the numpy restatement's bit for bit -- at 1 and 64 lights, one past the cap, with
spheres that do not emit among them, and behind a light triangle."""
import os

import numpy as np
import pytest

import spherelight_reference as R
import spherelight_support as S
from test_sanitizers import ENV, ROOT, built, run_clean  # noqa: F401  (built: the `make asan` fixture)

TRIANGLE = [-1.0, 4.0, -3.0, 2.0, 4.0, -3.5, 0.5, 4.5, -6.0]  # the driver's


@pytest.mark.parametrize("n, dark, with_triangle", [(1, 0, 0), (64, 0, 0), (1, 3, 1), (64, 5, 1), (65, 0, 0), (200, 0, 1), (3, 3, 1)])
def test_sphere_light_table_under_sanitizers(built, oracle, tmp_path, n, dark, with_triangle):
    rng = np.random.default_rng(100 + n + dark)
    rec = np.zeros((n + dark, 5))
    rec[:, :3] = rng.uniform(-8.0, 8.0, (n + dark, 3))
    rec[:, 3] = rng.uniform(0.01, 0.7, n + dark)
    rec[:, 4] = 5.0
    rec[rng.choice(n + dark, dark, replace=False), 4] = 0.0  # these do not emit
    if n == 3 and dark == 3:
        rec[:, 4] = 0.0  # none emits
    src, out = str(tmp_path / "spheres.bin"), str(tmp_path / "table.bin")
    rec.tofile(src)
    text = run_clean([os.path.join(built, "sphere_light_driver"), "table", str(len(rec)), src, str(with_triangle), out])
    head = text.split("\n")[0].split()
    rc, tris, spheres, kept, base, records = int(head[1]), int(head[3]), int(head[5]), int(head[7]), float.fromhex(head[9]), int(head[11])
    lit = rec[rec[:, 4] != 0.0]
    assert rc == 0 and tris == with_triangle and spheres == len(lit)
    assert kept == min(len(lit), 65)  # the list is kept up to one past the cap, the count runs on
    tab = R.table([TRIANGLE] if with_triangle else [], lit[:, :4])
    assert base == (tab.tri[-1, 13] if with_triangle else 0.0)
    got = np.fromfile(out).reshape(-1, 8)
    if 1 <= len(lit) <= 64:
        assert records == len(lit) and np.array_equal(S.bits(got), S.bits(tab.sph))
    else:
        assert records == 0 and got.size == 0
