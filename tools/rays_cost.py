#!/usr/bin/env python3
"""What ptx_render_rays_device and the lat-long projection cost.  Medians of 5 alternated runs after a warm-up:
wall clock around one call (each returns when its work is complete), one run of each setup in turn per round.  Fails without a GPU.

Rays: the camera rays of the Shirley 1080p frame, 8 passes (16.6 M rays), depth 8, one ray per bin, three ways:
  render_rays        ptx_render_rays_device on the rays ptx_camera_rays returns, at the samples' own offsets
  passes_identity    ptx_render_passes_device of the same 8 passes under the identity pose: the same samples through the same route
                     (generated rays, walk-first), so the difference is the generator's reads, the device check and the fold
  passes_off         the same passes as the benchmark renders them (no pose)
and the fold alone: ptx_render_rays_device at max_bounces = 0 (the check, one memset of the contributions and k_accum_rays; nothing is
generated or bounced) at 1, 64 and 256 rays per bin, beside the bytes it moves (32 B read per ray, 24 B read and written per bin, the
squares as much again) at the rate a float4 copy of the same run reaches.  k_generate_rays has no timer of its own (ptx_rays_params has
no time_kernels): its byte model (52 B read, 80 or 112 B written per ray) is recorded beside the call's time, not against a kernel time.

Panorama: Shirley 2048 x 1024, spp 64, depth 8 as a lat-long panorama against the identity-pose frame of the same sample count.

--parent-lib PATH: the benchmark against the parent commit (tools/texture_cost.py's A/B: alternated child processes of bench.py, the
parent's through PTX_LIB), recorded with the parent's own spread beside it.

usage: tools/rays_cost.py [--out profiles/pr_rays_cost.json] [--repeats 5] [--parent-lib PATH] [--small]"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from texture_cost import alternating_ms, headline_against_parent  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--small", action="store_true", help="a 480 x 270 frame and a 256 x 128 panorama at spp 8: checks the tool, measures nothing")
    ap.add_argument("--parent-lib", default=None, help="libptx_hip.so built from the parent commit: also run the headline A/B")
    a = ap.parse_args()
    headline = headline_against_parent(a.parent_lib, a.repeats) if a.parent_lib else None  # child processes first: this one has no GPU open yet
    import numpy as np
    import torch
    import path_tracer_ocaml_amd as P
    from path_tracer_ocaml_amd import host
    if P.lib().ptx_device_count() < 1:
        sys.exit("rays_cost: no GPU (nothing is measured on a CPU)")
    W, H, passes, depth = (480, 270, 8, 8) if a.small else (1920, 1080, 8, 8)
    res = {"width": W, "height": H, "passes": passes, "max_bounces": depth, "repeats": a.repeats}

    # ---- rays
    hs = host.shirley_spheres(W, H)
    g = P.Scene(hs.ptr, 0, keepalive=hs)
    ys, xs, ps = np.meshgrid(np.arange(H, dtype=np.int32), np.arange(W, dtype=np.int32), np.arange(passes, dtype=np.int32), indexing="ij")
    xs, ys, ps = xs.ravel(), ys.ravel(), ps.ravel()
    n = len(xs)
    o, d = g.camera_rays(W, H, passes, depth, xs, ys, ps)
    d_o, d_d = torch.tensor(o, device="cuda:0"), torch.tensor(d, device="cuda:0")
    d_off = torch.tensor((ys.astype(np.int64) * W + xs + ps.astype(np.int64) * passes).astype(np.int32), device="cuda:0")
    del o, d
    sums = torch.zeros((n, 3), dtype=torch.float64, device="cuda:0")
    sq = torch.zeros((n, 3), dtype=torch.float64, device="cuda:0")
    raw = torch.zeros((H, W, 3), dtype=torch.float64, device="cuda:0")
    params = P.render_params(W, H, passes, depth)
    posed = P.Scene(hs.ptr, 0, keepalive=hs)
    posed.set_camera_pose(np.zeros(3), np.eye(3))

    def rays(depth_, m, want_sq=False):
        return lambda: g.render_rays_device(n, d_o.data_ptr(), d_d.data_ptr(), sums.data_ptr(), d_off.data_ptr(), sq.data_ptr() if want_sq else None,
                                            max_bounces=depth_, rays_per_bin=m)
    got = alternating_ms({"render_rays": rays(depth, 1), "passes_identity": lambda: posed.render_passes_device(params, 0, passes, raw.data_ptr()),
                          "passes_off": lambda: g.render_passes_device(params, 0, passes, raw.data_ptr())}, a.repeats)
    for v in got.values():
        v["over_passes_identity_ms"] = v["median_ms"] - got["passes_identity"]["median_ms"]
    n_copy = (1 << 30) // 16 if not a.small else (1 << 24) // 16
    src = torch.zeros((n_copy, 4), dtype=torch.float32, device="cuda:0")
    dst = torch.empty_like(src)
    copy_runs = []
    for _ in range(a.repeats + 1):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        dst.copy_(src)
        torch.cuda.synchronize()
        copy_runs.append(time.perf_counter() - t0)
    rate = 2.0 * n_copy * 16 / statistics.median(copy_runs[1:])  # bytes moved per second: every byte is read and written
    del src, dst
    bins = [m for m in (1, 64, 256) if n % m == 0]
    fold = alternating_ms({f"m{m}{'_sq' if s else ''}": rays(0, m, s) for m in bins for s in (False, True)}, a.repeats)
    for key, v in fold.items():
        m, s = int(key[1:].split("_")[0]), key.endswith("_sq")
        moved = n * 32 + n * 32 + (n // m) * 48 * (2 if s else 1)  # the memset's writes, the fold's reads, the bins read and written
        v["bytes"] = moved
        v["byte_model_ms"] = moved / rate * 1e3
    res["rays"] = {"n": n, "setups": got, "float4_copy_bytes_per_s": rate,
                   "generator_byte_model": {"read_bytes_per_ray": 52, "written_bytes_per_ray": 80, "ms_at_copy_rate": n * 132 / rate * 1e3},
                   "fold_at_depth_0": fold}
    g.close()
    posed.close()
    del d_o, d_d, d_off, sums, sq, raw

    # ---- panorama
    PW, PH, spp = (256, 128, 8) if a.small else (2048, 1024, 64)
    hp = host.shirley_spheres(PW, PH)
    frames = {k: P.Scene(hp.ptr, 0, keepalive=hp) for k in ("latlong", "pose_identity")}
    frames["latlong"].set_camera_projection("latlong")
    frames["pose_identity"].set_camera_pose(np.zeros(3), np.eye(3))
    praw = torch.zeros((PH, PW, 3), dtype=torch.float64, device="cuda:0")
    pparams = P.render_params(PW, PH, spp, depth)
    pano = alternating_ms({k: (lambda s=s: s.render_raw_device(pparams, praw.data_ptr())) for k, s in frames.items()}, a.repeats)
    res["panorama"] = {"width": PW, "height": PH, "spp": spp, "setups": pano}
    for s in frames.values():
        s.close()
    if headline:
        res["unchanged_paths_against_parent"] = headline
    text = json.dumps(res, indent=1)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
