#!/usr/bin/env python3
"""What the feature passes and the a-trous filter cost on the GPU.  Medians of 5 after a warm-up, wall clock
around calls that end in a device synchronise; where two things are compared their runs alternate.  Fails without a GPU.

  (a) ptx_denoise_device alone at 1080p, levels 5, on seeded synthetic inputs -- per level against its byte model (96 B read and
      32 B written per pixel) as a fraction of the float4-copy rate of DESIGN.md section 5 (6.29 TB/s); and the tap-fetch A/B:
      gathers through L1 / L2 against the LDS-tiled variant (PTX_ATROUS_LDS = largest step served from LDS) at levels 1 and 2;
  (b) ptx_render_denoised on the Shirley scene at 1080p, spp 64, depth 8 against ptx_render_progressive with want_error, at
      K = 8 and K = 64 and at F = 8 and F = 0: the cost of the feature passes and of the filter per update;
  (c) (no GPU needed) the registers, spills and LDS of the new kernels are tools/kernel_resources.py's.

usage: tools/denoise_cost.py [--out FILE.json] [--width 1920 --height 1080 --spp 64 --depth 8 --repeats 5]"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
COPY_TBPS = 6.29  # float4 copy, DESIGN.md section 5


def median_ms(fn, repeats):
    fn()  # warm-up: code objects, workspaces
    out = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        fn()
        out.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(out), out


def alternating_ms(fns, repeats):
    """{name: (median, runs)} of several callables, one run of each in turn per round"""
    for f in fns.values():
        f()
    runs = {k: [] for k in fns}
    for _ in range(repeats):
        for k, f in fns.items():
            t0 = time.perf_counter()
            f()
            runs[k].append((time.perf_counter() - t0) * 1e3)
    return {k: (statistics.median(v), v) for k, v in runs.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--spp", type=int, default=64)
    ap.add_argument("--depth", type=int, default=8)
    ap.add_argument("--repeats", type=int, default=5)
    a = ap.parse_args()
    import torch
    import path_tracer_ocaml_amd as P
    from path_tracer_ocaml_amd import host
    if P.lib().ptx_device_count() < 1:
        sys.exit("denoise_cost: no GPU (nothing is measured on a CPU)")
    W, H = a.width, a.height
    npix = W * H
    res = {"width": W, "height": H, "spp": a.spp, "depth": a.depth, "repeats": a.repeats}

    # (a) the filter alone
    g = torch.Generator(device="cuda:0").manual_seed(1)
    k, kf = 8, 8
    raw = torch.rand((H, W, 3), dtype=torch.float64, device="cuda:0", generator=g) * k + 0.01
    err = torch.rand((H, W, 3), dtype=torch.float64, device="cuda:0", generator=g) + 1e-3
    feat = torch.rand((H, W, 8), dtype=torch.float64, device="cuda:0", generator=g) * kf
    feat[..., 7] = kf
    out = torch.zeros_like(raw)
    torch.cuda.synchronize()
    by_levels = {}
    for levels in (0, 1, 5):
        med, runs = median_ms(lambda: P.denoise_device(0, W, H, {"levels": levels}, k, kf, raw.data_ptr(), err.data_ptr(),
                                                       feat.data_ptr(), out.data_ptr()), a.repeats)
        by_levels[levels] = {"median_ms": med, "runs_ms": runs}
    per_level_ms = (by_levels[5]["median_ms"] - by_levels[1]["median_ms"]) / 4.0
    model_bytes = npix * (96 + 32)
    res["filter"] = {"by_levels": by_levels, "per_level_ms": per_level_ms, "model_bytes_per_level": model_bytes,
                     "model_ms_at_copy_rate": model_bytes / (COPY_TBPS * 1e12) * 1e3,
                     "fraction_of_copy_rate": (model_bytes / (COPY_TBPS * 1e12) * 1e3) / per_level_ms if per_level_ms > 0 else None}

    # the tap-fetch A/B, alternating runs: PTX_ATROUS_LDS = the largest step whose taps come from an LDS copy of the tile and its halo
    # (0: every step gathers through L1 / L2).  levels 1 = step 1, levels 2 = steps 1 and 2.
    default_lds = os.environ.get("PTX_ATROUS_LDS")

    def filt(lds_steps, levels):
        os.environ["PTX_ATROUS_LDS"] = str(lds_steps)
        P.denoise_device(0, W, H, {"levels": levels}, k, kf, raw.data_ptr(), err.data_ptr(), feat.data_ptr(), out.data_ptr())

    ab = alternating_ms({"gather_levels2": lambda: filt(0, 2), "lds_levels2": lambda: filt(2, 2), "lds_step1_levels2": lambda: filt(1, 2),
                         "gather_levels1": lambda: filt(0, 1), "lds_levels1": lambda: filt(1, 1)}, a.repeats)
    if default_lds is None:
        del os.environ["PTX_ATROUS_LDS"]
    else:
        os.environ["PTX_ATROUS_LDS"] = default_lds
    res["tap_fetch"] = {n: {"median_ms": m, "runs_ms": r} for n, (m, r) in ab.items()}

    # (b) the denoised render against the progressive one
    hs = host.shirley_spheres(W, H)
    scene = P.Scene(hs.ptr, 0, keepalive=hs)
    img = np.zeros((H, W, 3))
    renders = {}
    for K in (8, a.spp):
        fns = {"progressive": lambda K=K: scene.render_progressive(W, H, a.spp, a.depth, K, want_error=True, out=img)}
        for F in (8, 0):
            fns[f"denoised_F{F}"] = lambda K=K, F=F: scene.render_denoised(W, H, a.spp, a.depth, K, denoise={"feature_passes": F}, out=img)
        fns["denoised_F8_levels0"] = lambda K=K: scene.render_denoised(W, H, a.spp, a.depth, K, denoise={"feature_passes": 8, "levels": 0},
                                                                       out=img)
        got = alternating_ms(fns, a.repeats)
        renders[f"K{K}"] = {n: {"median_ms": m, "runs_ms": r} for n, (m, r) in got.items()}
    res["render"] = renders
    # the feature passes alone: 8 passes into a device buffer
    params = P.render_params(W, H, a.spp, a.depth)
    fbuf = torch.zeros((H, W, 8), dtype=torch.float64, device="cuda:0")
    med, runs = median_ms(lambda: scene.render_features_device(params, 0, 8, fbuf.data_ptr()), a.repeats)
    res["features_8_passes"] = {"median_ms": med, "runs_ms": runs}
    scene.close()
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
