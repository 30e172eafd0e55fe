"""The host half of the display rule (csrc/scene_host.cpp: display_check, display_thresholds, display_apply_host) under ASan + UBSan,
through the stand-alone driver tests/c/display_driver.cpp (`make asan`): every run exits 0 with nothing from the sanitizers on
stderr, the buffers are exactly as large as the rule says, and what the driver writes is the numpy restatement's bit for bit."""
import os

import numpy as np
import pytest

import display_reference as R
from test_sanitizers import ENV, ROOT, built, run_clean  # noqa: F401  (built: the `make asan` fixture)

LAYOUT = {"rgb8": ("uint8", 3), "rgba8": ("uint8", 4), "rgb32f": ("float32", 3), "rgba32f": ("float32", 4)}


@pytest.fixture(scope="module")
def T(built, tmp_path_factory):
    out = str(tmp_path_factory.mktemp("display") / "thresholds.bin")
    assert run_clean([os.path.join(built, "display_driver"), "thresholds", out]).split() == ["rc", "0", "doubles", "255"]
    t = np.fromfile(out)
    assert t.shape == (255,) and np.all(np.diff(t) > 0.0)
    return t


def test_threshold_construction_under_sanitizers_gives_the_librarys_table(T):
    import path_tracer_ocaml_amd as P
    assert np.array_equal(T.view(np.uint64), P.display_thresholds().view(np.uint64))


def _apply(built, tmp_path, img, fmt, transfer, tone, exposure):
    src, out = str(tmp_path / "rgb.bin"), str(tmp_path / "out.bin")
    np.ascontiguousarray(img, dtype=np.float64).tofile(src)
    text = run_clean([os.path.join(built, "display_driver"), "apply", str(R.FORMATS.index(fmt)), str(R.TRANSFERS.index(transfer)),
                      str(R.TONES.index(tone)), float(exposure).hex(), str(img.shape[0]), src, out])
    return text, out


@pytest.mark.parametrize("fmt", R.FORMATS)
def test_apply_under_sanitizers_on_edge_values_and_odd_sizes(built, T, tmp_path, fmt):
    dtype, ch = LAYOUT[fmt]
    images = [R.full_edge_image(T)] + [R.edge_image(T, n, seed=n) for n in (0, 1, 2, 3, 4, 5, 63, 64, 65, 257, 13 * 11)]
    todo = [s for s in R.settings() if s[0] == fmt]
    for i, (_, transfer, tone, exposure) in enumerate(todo):
        for img in (images if i < 2 else images[:1] + images[1 + i % 11:2 + i % 11]):
            text, out = _apply(built, tmp_path, img, fmt, transfer, tone, exposure)
            n = img.shape[0]
            assert text.split() == ["rc", "0", "bytes", str(n * ch * np.dtype(dtype).itemsize)]
            got = np.fromfile(out, dtype=dtype).reshape(n, ch)
            assert R.same(got, R.apply(img, T, fmt, transfer, tone, exposure)), (fmt, transfer, tone, exposure, n)


def test_refusals_under_sanitizers(built, tmp_path):
    img = np.zeros((2, 3))
    for args, message in ((("rgb8", "reference", "aces", 1.0), "PTX_TRANSFER_REFERENCE needs"),
                          (("rgb8", "reference", "none", 2.0), "PTX_TRANSFER_REFERENCE needs"),
                          (("rgb32f", "srgb", "none", 1.0), "binary32 formats"),
                          (("rgb8", "linear", "none", float("nan")), "exposure must be finite"),
                          (("rgb8", "linear", "none", -1.0), "exposure must be finite")):
        text, _ = _apply(built, tmp_path, img, *args)
        assert text.split("\n")[0] == "rc -1 bytes 0" and message in text, text
