#!/usr/bin/env python3
"""What the camera shutter costs over the posed frame.  Medians of 5 alternated runs after a warm-up: wall clock
around one ptx_render_raw_device of the frame (it returns when the frame is complete), one run of each setup in turn per round.
Fails without a GPU.

Two scenes at 1080p, spp 64, depth 8 -- the headline Shirley frame and the ganesha-like mesh (150 k triangles asked for, on a floor)
-- each under three camera states:
  pose           an oblique pose (tools/camera_pose_cost.py's)
  shutter        the same pose with a shutter that translates and turns
  lens_shutter   ... through a thin lens focused on the look-at target
and the generator's own time in a timed frame of each state (kernel by kernel: PTX_KERNEL_GENERATE).

The turntable: eight frames on a circle about the target's vertical axis over the mesh, on one handle, with and without a shutter
half of the way to the next frame's pose (the command line's --turntable=8 --shutter=0.5).

Reported, not barred: what a shutter may cost is not fixed in advance.

--parent-lib PATH: the benchmark against the parent commit (tools/texture_cost.py's A/B: alternated child processes of bench.py, the
parent's through PTX_LIB), recorded with the parent's own spread beside it.

usage: tools/shutter_cost.py [--out profiles/pr_shutter_cost.json] [--repeats 5] [--parent-lib PATH] [--small]"""
import argparse
import json
import os
import sys

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from camera_pose_cost import rodrigues, turntable_poses  # noqa: E402
from texture_cost import alternating_ms, headline_against_parent  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--parent-lib", default=None, help="libptx_hip.so built from the parent commit: also run the headline A/B")
    ap.add_argument("--small", action="store_true", help="a 480 x 270 frame, spp 8, and a 3 k mesh: checks the tool, measures nothing")
    a = ap.parse_args()
    headline = headline_against_parent(a.parent_lib, a.repeats) if a.parent_lib else None  # child processes first: this one has no GPU open yet
    import numpy as np
    import torch
    import path_tracer_ocaml_amd as P
    from path_tracer_ocaml_amd import host
    if P.lib().ptx_device_count() < 1:
        sys.exit("shutter_cost: no GPU (nothing is measured on a CPU)")
    W, H, spp, depth, n_tri = (480, 270, 8, 8, 3000) if a.small else (1920, 1080, 64, 8, 150000)
    raw = torch.zeros((H, W, 3), dtype=torch.float64, device="cuda:0")
    params = P.render_params(W, H, spp, depth)
    timed = P.render_params(W, H, spp, depth, time_kernels=True)
    res = {"width": W, "height": H, "spp": spp, "max_bounces": depth, "repeats": a.repeats}
    oblique = (0.9 * np.array([0.3, -0.2, 0.5]), rodrigues(np, (0.3, 1.0, 2.0), 0.15))
    axis = np.array([0.2, 0.9, -0.3])
    shutter = (np.array([0.3, 0.15, -0.35]), axis / np.linalg.norm(axis), 0.05)
    res["oblique_pose"] = {"origin": list(oblique[0]), "rotation": oblique[1].tolist()}
    res["shutter"] = {"translation": list(shutter[0]), "axis": list(shutter[1]), "angle": shutter[2]}

    # ---- a frame under three camera states
    def frame(hs):
        scenes = {k: P.Scene(hs.ptr, 0, keepalive=hs) for k in ("pose", "shutter", "lens_shutter")}
        for g in scenes.values():
            g.set_camera_pose(*oblique)
        scenes["shutter"].set_camera_shutter(*shutter)
        scenes["lens_shutter"].set_camera_shutter(*shutter)
        scenes["lens_shutter"].set_lens(0.05, hs.focus_distance)
        got = alternating_ms({k: (lambda g=g: g.render_raw_device(params, raw.data_ptr())) for k, g in scenes.items()}, a.repeats)
        for k, g in scenes.items():
            st = g.render_raw_device(timed, raw.data_ptr())
            got[k]["over_pose_ms"] = got[k]["median_ms"] - got["pose"]["median_ms"]
            got[k]["generate_kernel_ms"] = st["kernel_ms"]["generate"]
            got[k]["generate_launches"] = st["kernel_launches"]["generate"]
            got[k]["kernel_ms"] = st["kernel_ms"]
            g.close()
        return got
    hs = host.shirley_spheres(W, H)
    res["shirley"] = frame(hs)
    hm = host.ganesha_like(W, H, n_tri)
    res["mesh"] = dict(frame(hm), triangles=int(hm.d.n_triangles))

    # ---- the turntable, still and blurred
    n_frames, fraction = 8, 0.5
    poses = turntable_poses(np, host, hm, W / H, n_frames)
    motions = []
    for k in range(n_frames):
        nxt = poses[(k + 1) % n_frames]
        T, ax, angle = host.camera_shutter_between(poses[k][0], poses[k][1], nxt[0], nxt[1])
        motions.append((T * fraction, ax, angle * fraction))
    one = P.Scene(hm.ptr, 0, keepalive=hm)

    def still():
        one.set_camera_shutter(None)
        for pose in poses:
            one.set_camera_pose(*pose)
            one.render_raw_device(params, raw.data_ptr())

    def blurred():
        for pose, motion in zip(poses, motions):
            one.set_camera_pose(*pose)
            one.set_camera_shutter(*motion)
            one.render_raw_device(params, raw.data_ptr())
    tt = alternating_ms({"still": still, "shutter_0.5": blurred}, a.repeats)
    for v in tt.values():
        v["per_frame_ms"] = v["median_ms"] / n_frames
        v["over_still"] = v["median_ms"] / tt["still"]["median_ms"]
    res["turntable"] = {"frames": n_frames, "triangles": int(hm.d.n_triangles), "angle_between_frames": motions[0][2] / fraction, "ways": tt}
    one.close()
    if headline:
        res["bench_against_parent"] = headline
    text = json.dumps(res, indent=1)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
