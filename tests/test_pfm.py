"""The hosts' PFM reader (path_tracer_ocaml_amd/host/pfm.cpp): tiny files written here -- both byte orders, grey and colour, the
row order -- through libpt_host.so, and hostile files (truncated and malformed headers, short bodies) through the stand-alone
program tests/c/pfm_driver.cpp built with AddressSanitizer + UndefinedBehaviorSanitizer.  The command-line flags that use the reader
refuse what they must before any device is touched."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from test_sanitizers import built, run_clean  # noqa: F401  (built: the `make asan` fixture)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def write_pfm(path, img, little=True, scale=1.0, header=None):
    """img: (H, W, 3) or (H, W), row 0 = the BOTTOM row of the picture = the first row of the file"""
    img = np.asarray(img)
    magic = "PF" if img.ndim == 3 else "Pf"
    head = header if header is not None else "%s\n%d %d\n%s\n" % (magic, img.shape[1], img.shape[0], repr(-abs(scale) if little else abs(scale)))
    with open(path, "wb") as f:
        f.write(head.encode("ascii"))
        f.write(img.astype("<f4" if little else ">f4").tobytes())


def load(path):
    from path_tracer_ocaml_amd import host
    L = host.lib()
    L.pth_pfm_load.restype = C.c_void_p
    L.pth_pfm_load.argtypes = [C.c_char_p]
    L.pth_image_error.restype = C.c_char_p
    L.pth_image_rgb.restype = C.POINTER(C.c_double)
    for f in (L.pth_image_free, L.pth_image_width, L.pth_image_height, L.pth_image_channels, L.pth_image_rgb):
        f.argtypes = [C.c_void_p]
    h = L.pth_pfm_load(str(path).encode())
    if not h:
        return None, L.pth_image_error().decode()
    w, hh = L.pth_image_width(h), L.pth_image_height(h)
    rgb = np.ctypeslib.as_array(L.pth_image_rgb(h), shape=(hh, w, 3)).copy()
    ch = L.pth_image_channels(h)
    L.pth_image_free(h)
    return (rgb, ch), None


@pytest.mark.parametrize("little", [True, False])
@pytest.mark.parametrize("grey", [False, True])
def test_both_byte_orders_grey_and_colour_and_the_row_order(tmp_path, little, grey):
    rng = np.random.default_rng(3)
    img = rng.uniform(-2.0, 50.0, (3, 5) if grey else (3, 5, 3)).astype(np.float32)
    img[0, 0] = 1e-30  # the file's first value: texel (0, 0), v = 0
    p = tmp_path / "a.pfm"
    write_pfm(p, img, little=little, scale=2.5)
    (rgb, ch), err = load(p)
    assert err is None and ch == (1 if grey else 3) and rgb.shape == (3, 5, 3)
    want = np.repeat(img[:, :, None], 3, axis=2) if grey else img
    assert np.array_equal(rgb, want.astype(np.float64))  # binary32 -> binary64 unchanged, the scale's magnitude not applied
    assert rgb[0, 0, 0] == np.float64(np.float32(1e-30))  # rows are kept as they come: the file's first row is row 0


def test_header_white_space_is_free_but_one_byte_ends_it(tmp_path):
    img = np.arange(12, dtype=np.float32).reshape(2, 2, 3)
    p = tmp_path / "a.pfm"
    write_pfm(p, img, header="PF 2\t2\r\n-1\n")
    (rgb, _), err = load(p)
    assert err is None and np.array_equal(rgb, img)
    # a pixel byte that happens to be white space is data: 0x20 0x20 0x20 0x20 is a valid float
    with open(p, "wb") as f:
        f.write(b"Pf\n1 1\n-1.0\n" + b"    ")
    (rgb, _), err = load(p)
    assert err is None and rgb[0, 0, 0] == np.float64(np.frombuffer(b"    ", dtype="<f4")[0])


HOSTILE = [
    (b"", "start with"), (b"P", "start with"), (b"PG\n1 1\n-1\n\0\0\0\0", "start with"), (b"P6\n1 1\n255\n\0\0\0", "start with"),
    (b"PF", "magic"), (b"PFX\n1 1\n-1\n", "magic"), (b"PF\n", "width and height"), (b"PF\n3", "width and height"), (b"PF\n3 ", "width and height"),
    (b"PF\n3 2", "width and height"), (b"PF\nx 2\n-1\n", "integers"), (b"PF\n2.5 2\n-1\n", "integers"),
    (b"PF\n0 2\n-1\n", "must be in [1, 16384]"), (b"PF\n2 -2\n-1\n", "must be in [1, 16384]"), (b"PF\n16385 1\n-1\n", "must be in [1, 16384]"),
    (b"PF\n99999999999999999999 1\n-1\n", "must be in [1, 16384]"), (b"PF\n" + b"9" * 64 + b" 1\n-1\n", "width and height"),
    (b"PF\n2 2\n", "scale"), (b"PF\n2 2\n-1.0", "scale"), (b"PF\n2 2\n0\n" + b"\0" * 48, "finite non-zero"), (b"PF\n2 2\nnan\n" + b"\0" * 48, "finite non-zero"),
    (b"PF\n2 2\ninf\n" + b"\0" * 48, "finite non-zero"), (b"PF\n2 2\n-1e\n" + b"\0" * 48, "finite non-zero"),
    (b"PF\n2 2\n-1\n", "ends early"), (b"PF\n2 2\n-1\n" + b"\0" * 47, "ends early"), (b"Pf\n2 2\n-1\n" + b"\0" * 15, "ends early"),
    (b"PF\n16384 16384\n-1\n" + b"\0" * 64, "ends early"),
    (b"Pf\n2 1\n-1\n" + np.array([1.0, np.nan], dtype="<f4").tobytes(), "pixel (1, 0) is not finite"),
    (b"Pf\n1 2\n1\n" + np.array([1.0, np.inf], dtype=">f4").tobytes(), "pixel (0, 1) is not finite"),
]


def test_reader_on_hostile_files_under_the_sanitizers(built, tmp_path):  # noqa: F811
    exe = os.path.join(built, "pfm_driver")
    good = tmp_path / "good.pfm"
    img = np.arange(24, dtype=np.float32).reshape(2, 4, 3)
    write_pfm(good, img, little=False)
    paths = [str(good), str(tmp_path / "missing.pfm")]
    for k, (data, _) in enumerate(HOSTILE):
        p = tmp_path / ("bad%02d.pfm" % k)
        p.write_bytes(data)
        paths.append(str(p))
    lines = run_clean([exe] + paths).splitlines()  # exit 0, nothing from the sanitizers
    assert len(lines) == len(paths)
    head = lines[0].split()
    assert head[:4] == ["ok", "4", "2", "3"] and [float.fromhex(v) for v in head[4:]] == img.ravel().tolist()
    assert lines[1].startswith("error PFM: cannot open")
    for line, (data, want) in zip(lines[2:], HOSTILE):
        assert line.startswith("error PFM: ") and want in line, (data[:24], line)


def test_library_and_driver_refuse_alike(tmp_path):
    for k, (data, want) in enumerate(HOSTILE[:8]):
        p = tmp_path / ("bad%d.pfm" % k)
        p.write_bytes(data)
        got, err = load(p)
        assert got is None and want in err


def test_cli_refuses_bad_image_flags_before_any_device(tmp_path):
    exe = os.path.join(ROOT, "path_tracer_ocaml_amd", "shirley_spheres")
    bad = tmp_path / "bad.pfm"
    bad.write_bytes(b"PF\n2 2\n-1\n")
    for flags, code, want in ((["--envmap="], 124, "expected a PFM file"), (["--envmap-rotate=ten", "--envmap=x.pfm"], 124, "expected degrees"),
                              (["--texture-nearest"], 124, "requires --ground-texture"), (["--envmap-rotate=10"], 124, "requires --envmap")):
        r = subprocess.run([exe, "--dimension=16,8"] + flags, capture_output=True, text=True)
        assert r.returncode == code and want in r.stderr, (flags, r.stderr)
    r = subprocess.run([exe, "--dimension=16,8", "--scene=cornell", "--ground-texture=x.pfm"], capture_output=True, text=True)
    assert r.returncode == 124 and "no ground or floor material" in r.stderr
    for name in ("cornell_box", "ganesha"):
        for flags, want in ((["--envmap-rotate=ten"], "expected degrees"), (["--texture-nearest"], "requires --ground-texture"),
                            (["--envmap-rotate=10"], "requires --envmap")):
            r = subprocess.run([os.path.join(ROOT, "path_tracer_ocaml_amd", name)] + flags, capture_output=True, text=True)
            assert r.returncode == 2 and want in r.stderr, (name, flags, r.stderr)
        r = subprocess.run([os.path.join(ROOT, "path_tracer_ocaml_amd", name), "-help"], capture_output=True, text=True)
        assert r.returncode == 0 and "--envmap=FILE.pfm" in r.stdout and "no pixel sees it" in r.stdout
    r = subprocess.run([os.path.join(ROOT, "path_tracer_ocaml_amd", "cornell_box"), "--ground-texture=x.pfm"], capture_output=True, text=True)
    assert r.returncode == 2 and "no ground or floor material" in r.stderr
    from path_tracer_ocaml_amd import host
    L = host.lib()
    R = (C.c_double * 9)()
    L.pth_rotation_y.argtypes = [C.c_double, C.POINTER(C.c_double)]
    L.pth_rotation_y(90.0, R)
    assert np.allclose(np.array(list(R)).reshape(3, 3), [[0, 0, 1], [0, 1, 0], [-1, 0, 0]], atol=1e-15)
    L.pth_ground_texture.argtypes = [C.c_void_p]
    assert L.pth_ground_texture(C.cast(host.shirley_spheres(16, 8).ptr, C.c_void_p)) == 0
