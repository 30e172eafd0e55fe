#!/usr/bin/env python3
"""Host cost of the camera tile lists (csrc/scene_host.cpp: scene_tile_lists): time to build the grid of the Shirley scene and its size.
Builds tests/c/tile_lists_driver.cpp as a plain -O2 program (the flags of host/Makefile, no sanitizer) and runs its `grid` mode.
The build runs once per (scene, image size), at the first render of that size; bench.py's warm-up step absorbs it.
usage: tools/tile_lists_cost.py [WxH ...]   (default 1920x1080 3840x2160)"""
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "path_tracer_ocaml_amd", "host")
CSRC = os.path.join(ROOT, "path_tracer_ocaml_amd", "csrc")
sizes = [tuple(int(v) for v in a.split("x")) for a in sys.argv[1:]] or [(1920, 1080), (3840, 2160)]
with tempfile.TemporaryDirectory() as tmp:
    exe = os.path.join(tmp, "tile_lists_driver")
    src = [os.path.join(ROOT, "tests", "c", "tile_lists_driver.cpp")] + [os.path.join(HOST, f) for f in ("scenes.cpp", "png_write.cpp", "ply.cpp", "ppm_command.cpp")] + \
          [os.path.join(CSRC, f) for f in ("bvh_build.cpp", "scene_host.cpp")]
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-march=x86-64-v3", "-ffp-contract=off", "-fno-fast-math", "-fno-math-errno", "-o", exe] + src)
    for w, h in sizes:
        best = None
        for _ in range(5):
            f = subprocess.run([exe, "grid", "shirley", str(w), str(h), tmp], capture_output=True, text=True, check=True).stdout.split()
            info = {f[i]: f[i + 1] for i in range(0, 16, 2)}
            best = min(best or 1e30, int(info["build_us"]))
        tiles = int(info["tiles_x"]) * int(info["tiles_y"])
        print(f"{w}x{h}: {tiles} tiles, {tiles * 32} bytes ({tiles * 32 / 1e6:.2f} MB), {info['walk']} walk tiles, longest list {info['longest']}, "
              f"built in {best / 1000:.2f} ms (best of 5, one thread)")
