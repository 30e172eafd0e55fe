#!/usr/bin/env python3
"""What the lighting modes cost and buy: the lamp scene (cornell with a square lamp of half side 0.03 at y = 0.999, emit 400,
ceiling black) at 1024 x 1024, spp 256, depth 16, rendered in modes 0, 1 and 2 of one scene handle, alternated in one process;
medians of `reps` runs.  Per mode: ms per frame (ptx_render into a pinned image) and, from one ptx_render_progressive run's error
image, the median per-pixel standard error (mean of r, g, b); and the time each mode would need to reach mode 2's median error,
standard error falling as 1 / sqrt(passes).  One JSON line.
Usage: lighting_cost.py [reps] [width] [spp]"""
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402

import path_tracer_ocaml_amd as P  # noqa: E402
from path_tracer_ocaml_amd import abi, host as H  # noqa: E402

DEPTH = 16


def timed(fn):
    t0 = time.perf_counter()
    fn()
    return (time.perf_counter() - t0) * 1e3


def main():
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 5
    w = h = int(sys.argv[2]) if len(sys.argv) > 2 else 1024
    spp = int(sys.argv[3]) if len(sys.argv) > 3 else 256
    hs = H.cornell_lamp(w, h, 0.0, 0.03, 0.999, 400.0)
    sc = P.Scene(hs.ptr, 0, keepalive=hs)
    img = np.zeros((h, w, 3))
    sc.pin_image(img)
    modes = (0, 1, 2)
    runs = {m: [] for m in modes}

    def run(m):
        sc.set_lighting(m)
        return timed(lambda: sc.render(w, h, spp, DEPTH, out=img))

    for m in modes:  # warm-up: workspaces, staging, first launches of each mode's kernels
        run(m)
    for _ in range(reps):
        for m in modes:  # alternated, so drift hits every mode alike
            runs[m].append(run(m))
    sc.unpin_image()
    err = {}
    for m in modes:  # the error image of the whole frame (one update at the end)
        sc.set_lighting(m)
        _, e, done, _ = sc.render_progressive(w, h, spp, DEPTH, spp, want_error=True)
        assert done == spp
        per_pixel = e.mean(axis=2)
        err[m] = {"median": float(np.median(per_pixel)), "zero_pixels": int((per_pixel == 0.0).sum())}
    ms = {m: statistics.median(runs[m]) for m in modes}
    target = err[2]["median"]
    out = {"scene": "cornell_lamp(0.03, 0.999, 400)", "width": w, "height": h, "spp": spp, "depth": DEPTH, "reps": reps, "modes": {}}
    for m in modes:
        e = err[m]["median"]
        out["modes"][abi.PTX_LIGHTING_NAMES[m]] = {
            "ms": round(ms[m], 3), "over_reference": round(ms[m] / ms[0] - 1, 4), "median_pixel_stderr": e,
            "pixels_with_zero_error": err[m]["zero_pixels"],
            # passes scale with (e / target)^2; a median of 0 (most pixels saw no light at all) has no such estimate
            "ms_to_sampled_error": round(ms[m] * (e / target) ** 2, 1) if e > 0.0 and target > 0.0 else None,
        }
    print(json.dumps(out), flush=True)
    sc.close()


if __name__ == "__main__":
    main()
