#!/usr/bin/env python3
"""What temporal accumulation costs.  Medians of 5 alternated runs after a warm-up.  Fails without a GPU.

The kernel alone, at 1080p and 4K, against its byte model.  The inputs make every pixel take history with all four taps accepted
(a wall at one depth, a camera turned about its own origin by a fraction of a degree): the most traffic the rule can ask for.
  call_ms     wall clock around ptx_temporal_accumulate_device (it returns when the stream is idle): the launch, a one-word
              allocation, its memset and copy, and the wait -- 20 calls per timed window
  device_ms   device events around the same calls on the same stream: the memset, the kernel and the 8-byte copy
  byte model  per pixel, reads 48 (sums and square sums) + 64 (features) + the history taps, writes 96 + 48, plus 24 with motion;
              "every_tap": four 96-byte taps per pixel, as if no tap were shared; "compulsory": each history record once
  at the rate a float4 copy of 1 GiB reaches in the same run (a copy moves every byte twice).  These are bounds, not predictions.

A turntable frame: the ganesha-like mesh (150 k triangles asked for, on a floor) at 1080p, depth 8, eight frames over an arc of
8 degrees, one scene handle per way, every way into the same host image (a fresh 50 MB image per frame costs a millisecond of page
faults, which is not the library's), per-frame medians:
  temporal            ptx_render_temporal, 8 passes a frame out of a sequence of 64
  temporal_denoised   the same with the default a-trous filter on the accumulated frame
  denoised_spp8       ptx_render_denoised at spp 8, one update
  plain_spp8          ptx_render at spp 8: what a temporal frame adds its features, its accumulation and its error to
  plain_spp64         ptx_render at spp 64: the frame a sequence of eight temporal frames has as many samples as

--parent-lib PATH: bench.py's headline against the parent commit (tools/texture_cost.py's A/B: alternated child processes, the
parent's library through PTX_LIB), with the parent's own spread beside it.

usage: tools/temporal_cost.py [--out profiles/pr_temporal_cost.json] [--repeats 5] [--parent-lib PATH] [--small]"""
import argparse
import json
import math
import os
import statistics
import sys
import time

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from camera_pose_cost import rodrigues  # noqa: E402
from texture_cost import alternating_ms, headline_against_parent  # noqa: E402

CALLS = 20  # per timed window of the kernel alone


def kernel_alone(np, torch, P, abi, W, H, repeats, copy_rate):
    n = W * H
    dev = "cuda:0"
    k = kf = 8
    view = (-(W / H) * 0.4, -0.4, 2.0 * (W / H) * 0.4, 0.8)
    cur = abi.temporal_camera(np.zeros(3), np.eye(3), view)
    prev = abi.temporal_camera(np.zeros(3), rodrigues(np, (0.2, 1.0, 0.0), math.radians(0.25)), view)
    g = torch.Generator(device=dev).manual_seed(1)
    raw = torch.rand((n, 3), dtype=torch.float64, device=dev, generator=g) * k
    sq = raw * raw / k + torch.rand((n, 3), dtype=torch.float64, device=dev, generator=g) * k
    z = 5.0
    feat = torch.zeros((n, 8), dtype=torch.float64, device=dev)
    feat[:, 0:3] = 0.5 * kf
    feat[:, 5] = float(kf)       # the wall's normal (0, 0, 1), summed
    feat[:, 6] = z * kf
    feat[:, 7] = float(kf)
    hist = torch.zeros((n, 12), dtype=torch.float64, device=dev)
    hist[:, 0:3] = torch.rand((n, 3), dtype=torch.float64, device=dev, generator=g)
    hist[:, 3:6] = hist[:, 0:3] ** 2 + 0.1
    hist[:, 6] = 24.0
    hist[:, 7] = 1.0
    hist[:, 10] = 1.0
    hist[:, 11] = z
    out_h, out_r, out_e, out_m = (torch.zeros((n, c), dtype=torch.float64, device=dev) for c in (12, 3, 3, 3))
    took = {}

    def run(motion):
        def f():
            for _ in range(CALLS):
                took[motion] = P.temporal_accumulate_device(0, W, H, None, k, kf, cur, prev, raw.data_ptr(), sq.data_ptr(), feat.data_ptr(),
                                                            hist.data_ptr(), out_h.data_ptr(), out_r.data_ptr(), out_e.data_ptr(),
                                                            out_m.data_ptr() if motion else None)
        return f
    wall = alternating_ms({"without_motion": run(False), "with_motion": run(True)}, repeats)
    res = {}
    for name, motion in (("without_motion", False), ("with_motion", True)):
        ev = []
        for _ in range(repeats + 1):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            run(motion)()
            b.record()
            b.synchronize()
            ev.append(a.elapsed_time(b) / CALLS)
        every_tap = 48 + 64 + 4 * 96 + 96 + 48 + (24 if motion else 0)
        compulsory = 48 + 64 + 96 + 96 + 48 + (24 if motion else 0)
        device_ms = statistics.median(ev[1:])
        res[name] = {"call_ms": wall[name]["median_ms"] / CALLS, "call_runs_ms": [v / CALLS for v in wall[name]["runs_ms"]],
                     "device_ms": device_ms, "device_runs_ms": ev[1:], "history_pixels": int(took[motion]), "pixels": n,
                     "bytes_per_pixel": {"every_tap": every_tap, "compulsory": compulsory},
                     "byte_model_ms": {"every_tap": n * every_tap / copy_rate * 1e3, "compulsory": n * compulsory / copy_rate * 1e3},
                     "device_bytes_per_s": {"every_tap": n * every_tap / (device_ms * 1e-3), "compulsory": n * compulsory / (device_ms * 1e-3)}}
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--parent-lib", default=None, help="libptx_hip.so built from the parent commit: also run the headline A/B")
    ap.add_argument("--small", action="store_true", help="480 x 270 frames and a 3 k mesh: checks the tool, measures nothing")
    a = ap.parse_args()
    headline = headline_against_parent(a.parent_lib, a.repeats) if a.parent_lib else None  # child processes first: this one has no GPU open yet
    note = lambda what: print("temporal_cost: " + what, file=sys.stderr, flush=True)  # noqa: E731
    note("headline A/B done" if headline else "no headline A/B asked for")
    import numpy as np
    import torch
    import path_tracer_ocaml_amd as P
    from path_tracer_ocaml_amd import abi, host
    if P.lib().ptx_device_count() < 1:
        sys.exit("temporal_cost: no GPU (nothing is measured on a CPU)")
    res = {"repeats": a.repeats, "calls_per_window": CALLS}

    # ---- the rate of a float4 copy in this run
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
    copy_rate = 2.0 * n_copy * 16 / statistics.median(copy_runs[1:])  # bytes moved per second: every byte is read and written
    del src, dst
    res["float4_copy_bytes_per_s"] = copy_rate
    note("copy rate %.3g B/s" % copy_rate)

    # ---- the kernel alone
    sizes = {"480x270": (480, 270)} if a.small else {"1080p": (1920, 1080), "4k": (3840, 2160)}
    res["kernel"] = {name: kernel_alone(np, torch, P, abi, w, h, a.repeats, copy_rate) for name, (w, h) in sizes.items()}

    note("kernel alone done")

    # ---- a turntable frame
    W, H, depth, n_tri = (480, 270, 8, 3000) if a.small else (1920, 1080, 8, 150000)
    S, frames = 8, 8
    hm = host.ganesha_like(W, H, n_tri)
    cam = hm.camera
    up = cam["up"] / np.linalg.norm(cam["up"])
    arm = cam["eye"] - cam["target"]
    poses = [host.camera_pose_look_at(cam["look_at"], cam["target"] + rodrigues(np, up, math.radians(8.0) * k / frames) @ arm, cam["target"],
                                      cam["up"], W / H, cam["fov_deg"]) for k in range(frames)]
    ways = ("temporal", "temporal_denoised", "denoised_spp8", "plain_spp8", "plain_spp64")
    scenes = {w: P.Scene(hm.ptr, 0, keepalive=hm) for w in ways}
    out = np.zeros((H, W, 3))
    shares = {"temporal": [], "temporal_denoised": []}

    def sequence(way):
        g = scenes[way]

        def run():
            if way.startswith("temporal"):
                g.temporal_reset()
            for k, pose in enumerate(poses):
                g.set_camera_pose(*pose)
                if way.startswith("temporal"):
                    took = g.render_temporal(W, H, S * frames, depth, k * S, S, denoise=True if way.endswith("denoised") else None, out=out)[3]
                    if k:
                        shares[way].append(took / (W * H))
                elif way == "denoised_spp8":
                    g.render_denoised(W, H, S, depth, S, out=out)
                else:
                    g.render(W, H, S if way == "plain_spp8" else S * frames, depth, out=out)
        return run
    note("scenes built")
    got = alternating_ms({w: sequence(w) for w in ways}, a.repeats)
    note("turntable done")
    for w, v in got.items():
        v["per_frame_ms"] = v["median_ms"] / frames
        v["over_plain_spp8_ms"] = v["per_frame_ms"] - got["plain_spp8"]["median_ms"] / frames
    for w, v in shares.items():
        got[w]["history_share_min_max"] = [min(v), max(v)]
    res["turntable"] = {"width": W, "height": H, "max_bounces": depth, "frames": frames, "passes_per_frame": S, "arc_degrees": 8.0,
                        "triangles": int(hm.d.n_triangles), "ways": got}
    for g in scenes.values():
        g.close()
    if headline:
        res["headline_against_parent"] = headline
    text = json.dumps(res, indent=1)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
