#!/usr/bin/env python3
"""What the thin-lens camera costs.  Medians of 5 alternated runs after a warm-up: wall clock around one
ptx_render_raw_device of the frame (it returns when the frame is complete), one run of each setup in turn per round.  Fails without a
GPU.

The headline frame (Shirley 1080p, spp 64, depth 8) and the ganesha-like frame (150 k triangles on a floor, walked from HBM / L2), each
under three setups:
  lens_off         the scene as the benchmark renders it: the pinhole's own path (Shirley: shade-first order, per-octant LDS image,
                   camera tile lists)
  lens_off_walk    the same with PTX_BOUNCE_ORDER=0: the walk-first schedule a lens render takes, without a lens -- what of the
                   difference below is the SCHEDULE
  lens_on          a lens: Shirley at the book's aperture 0.1 (radius 0.05) focused at 10; the mesh at radius focus / 200, focused on
                   the camera's look-at target
lens_on against lens_off_walk is what writing the camera rays into HBM and reading them back costs.  Reported, not barred.

--parent-lib PATH: the pinhole against the parent commit (tools/texture_cost.py's A/B: alternated child processes of bench.py, the
parent's through PTX_LIB), recorded with the parent's own spread beside it.

usage: tools/lens_cost.py [--out profiles/pr_thin_lens_cost.json] [--repeats 5] [--parent-lib PATH] [--small]"""
import argparse
import json
import os
import sys

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from texture_cost import alternating_ms, headline_against_parent, scene_with_env  # noqa: E402

WALK_FIRST = {"PTX_BOUNCE_ORDER": "0"}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--parent-lib", default=None, help="libptx_hip.so built from the parent commit: also run the headline A/B")
    ap.add_argument("--small", action="store_true", help="a 480 x 270 frame, spp 8, and a 3 k mesh: checks the tool, measures nothing")
    a = ap.parse_args()
    headline = headline_against_parent(a.parent_lib, a.repeats) if a.parent_lib else None  # child processes first: this one has no GPU open yet
    import torch
    import path_tracer_ocaml_amd as P
    from path_tracer_ocaml_amd import host
    if P.lib().ptx_device_count() < 1:
        sys.exit("lens_cost: no GPU (nothing is measured on a CPU)")
    W, H, spp, depth, n_tri = (480, 270, 8, 8, 3000) if a.small else (1920, 1080, 64, 8, 150000)
    raw = torch.zeros((H, W, 3), dtype=torch.float64, device="cuda:0")
    params = P.render_params(W, H, spp, depth)
    res = {"width": W, "height": H, "spp": spp, "max_bounces": depth, "repeats": a.repeats, "frames": {}}

    def frame(g):
        return lambda: g.render_raw_device(params, raw.data_ptr())

    def measure(hs, lens):
        scenes = {"lens_off": P.Scene(hs.ptr, 0, keepalive=hs), "lens_off_walk": scene_with_env(P, hs, WALK_FIRST),
                  "lens_on": P.Scene(hs.ptr, 0, keepalive=hs)}
        scenes["lens_on"].set_lens(*lens)
        got = alternating_ms({k: frame(g) for k, g in scenes.items()}, a.repeats)
        for v in got.values():
            v["over_lens_off_ms"] = v["median_ms"] - got["lens_off"]["median_ms"]
            v["over_lens_off_walk_ms"] = v["median_ms"] - got["lens_off_walk"]["median_ms"]
        # where the lens render's time goes, by kernel kind (one timed frame: the events serialise the two streams)
        timed = P.render_params(W, H, spp, depth, time_kernels=True)
        st = scenes["lens_on"].render_raw_device(timed, raw.data_ptr())
        for g in scenes.values():
            g.close()
        return {"lens": {"radius": lens[0], "focus_distance": lens[1]}, "setups": got,
                "lens_on_kernel_ms": st["kernel_ms"], "lens_on_kernel_launches": st["kernel_launches"]}

    res["frames"]["shirley"] = measure(host.shirley_spheres(W, H), (0.05, 10.0))
    hm = host.ganesha_like(W, H, n_tri)
    res["frames"]["ganesha_like"] = dict(measure(hm, (hm.focus_distance / 200.0, hm.focus_distance)), triangles=n_tri)
    if headline:
        res["pinhole_against_parent"] = headline
    text = json.dumps(res, indent=1)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
