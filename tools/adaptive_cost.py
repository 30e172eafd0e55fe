#!/usr/bin/env python3
"""What adaptive sampling costs and buys: ptx_render_adaptive on bench.py's headline frame and its cornell configuration, one JSON
line per run.  Each line records the time, the samples, the rounds and each round's list length; the time per sample of list rounds
against full-frame slices (ptx_render_pixels_device over all pixels against ptx_render_passes_device, K passes); for T = 0 the time
against ptx_render_progressive (K, want_error); and equal-sample quality: the RMSE against a 4N-pass ptx_render frame, next to the
RMSE of ptx_render at the uniform spp with the same total samples.
Usage: adaptive_cost.py [reps] [frames...]  (frames: shirley_1080p, cornell_1024)"""
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402

import path_tracer_ocaml_amd as P  # noqa: E402
from path_tracer_ocaml_amd import host as H  # noqa: E402

FRAMES = {  # name: (scene builder, width, height, spp, depth) -- as tools/progressive_cost.py
    "shirley_1080p": (lambda w, h: H.shirley_spheres(w, h), 1920, 1080, 64, 8),
    "cornell_1024": (lambda w, h: H.cornell_box(w, h), 1024, 1024, 256, 16),
}
M = K = 8
TARGETS = (0.0, 0.05, 0.02)


def timed(fn):
    t0 = time.perf_counter()
    out = fn()
    return (time.perf_counter() - t0) * 1e3, out


def rmse(a, b):
    return float(np.sqrt(np.mean((a - b) ** 2)))


def per_sample_ms(torch, sc, w, h, spp, depth, reps):
    """ms per sample of K passes [M, M + K) as a full-frame slice and as a list of every pixel, medians of `reps`"""
    params = P.render_params(w, h, spp, depth)
    raw = torch.zeros((h, w, 3), dtype=torch.float64, device="cuda:0")
    sq = torch.zeros_like(raw)
    lst = torch.arange(w * h, dtype=torch.int32, device="cuda:0")
    n = w * h * K
    slice_ms, list_ms = [], []
    for r in range(reps + 1):
        torch.cuda.synchronize()
        a, _ = timed(lambda: sc.render_passes_device(params, M, K, raw.data_ptr(), sq.data_ptr()))
        b, _ = timed(lambda: sc.render_pixels_device(params, M, K, lst.data_ptr(), w * h, raw.data_ptr(), sq.data_ptr()))
        if r:  # the first pair warms the workspaces up
            slice_ms.append(a)
            list_ms.append(b)
    return statistics.median(slice_ms) / n * 1e6, statistics.median(list_ms) / n * 1e6  # ns per sample


def main():
    import torch
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 3
    names = sys.argv[2:] or list(FRAMES)
    for name in names:
        build, w, h, spp, depth = FRAMES[name]
        hs = build(w, h)
        sc = P.Scene(hs.ptr, 0, keepalive=hs)
        img = np.zeros((h, w, 3))
        sc.pin_image(img)
        ref, _ = sc.render(w, h, 4 * spp, depth)  # the quality yardstick
        slice_ns, list_ns = per_sample_ms(torch, sc, w, h, spp, depth, reps)
        for T in TARGETS:
            rounds = []
            sc.render_adaptive(w, h, spp, depth, T, min_passes=M, passes_per_round=K, out=img)  # warm-up
            runs = []
            for _ in range(reps):
                rounds.clear()
                ms, (rgb, _, passes, st) = timed(lambda: sc.render_adaptive(
                    w, h, spp, depth, T, min_passes=M, passes_per_round=K, out=img,
                    on_round=lambda r, b, act, smp, rel, *a: rounds.append((b, act))))
                runs.append(ms)
            total = int(passes.sum())
            uni_spp = max(1, int(round(total / (w * h))))
            uni, _ = sc.render(w, h, uni_spp, depth)
            out = {"frame": name, "width": w, "height": h, "spp": spp, "depth": depth, "reps": reps, "min_passes": M,
                   "passes_per_round": K, "target": T, "ms": round(statistics.median(runs), 3), "samples": total,
                   "samples_frac": round(total / (w * h * spp), 4), "rounds": len(rounds),
                   "list_lengths": [w * h] + [a for _, a in rounds[:-1]],
                   "ns_per_sample_slice": round(slice_ns, 4), "ns_per_sample_list": round(list_ns, 4),
                   "rmse_adaptive": rmse(img, ref), "uniform_spp": uni_spp, "rmse_uniform": rmse(uni, ref)}
            if T == 0.0:
                prog = []
                for _ in range(reps):
                    ms, _ = timed(lambda: sc.render_progressive(w, h, spp, depth, K, want_error=True, out=img))
                    prog.append(ms)
                out["progressive_ms"] = round(statistics.median(prog), 3)
                out["over_progressive"] = round(out["ms"] / out["progressive_ms"] - 1, 4)
            print(json.dumps(out), flush=True)
        sc.unpin_image()
        sc.close()


if __name__ == "__main__":
    main()
