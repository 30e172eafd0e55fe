#!/usr/bin/env python3
"""What the camera pose costs, and what it saves.  Medians of 5 alternated runs after a warm-up: wall clock
around one ptx_render_raw_device of the frame (it returns when the frame is complete), one run of each setup in turn per round.
Fails without a GPU.

The headline frame (Shirley 1080p, spp 64, depth 8) three ways:
  pose_off       the scene as the benchmark renders it (shade-first order, per-octant LDS image, camera tile lists)
  pose_identity  the identity pose at origin 0: the same picture bit for bit through the posed route (generated rays, walk-first)
  pose_oblique   a camera moved and turned (tests/camera_pose_support.py's oblique pose)
and the generator's own time in a timed frame of pose_oblique against its byte model: entries x record bytes at the rate a float4
copy of the same run reaches (torch's device-to-device copy of 1 GiB; a copy moves every byte twice, the generator only writes).

The turntable: eight frames on a circle about the target's vertical axis over the ganesha-like mesh (150 k triangles asked for, on
a floor) at 1080p, spp 64, depth 8, two ways:
  set_pose       ptx_scene_set_camera_pose + render on one handle
  rebuild        destroy / create / render per frame, with the host and with the GPU BVH builder (the vertices are NOT transformed
                 again here, so this side is flattered)
The ratio is the feature's reason to exist.  Reported, not barred.

--parent-lib PATH: the unposed benchmark against the parent commit (tools/texture_cost.py's A/B: alternated child processes of
bench.py, the parent's through PTX_LIB), recorded with the parent's own spread beside it.

usage: tools/camera_pose_cost.py [--out profiles/pr_camera_pose_cost.json] [--repeats 5] [--parent-lib PATH] [--small]"""
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
from texture_cost import alternating_ms, headline_against_parent  # noqa: E402


def rodrigues(np, axis, angle):
    a = np.asarray(axis, dtype=np.float64)
    a = a / np.linalg.norm(a)
    K = np.array([[0.0, -a[2], a[1]], [a[2], 0.0, -a[0]], [-a[1], a[0], 0.0]])
    return np.eye(3) + math.sin(angle) * K + (1.0 - math.cos(angle)) * (K @ K)


def turntable_poses(np, host, hs, aspect, n):
    """n cameras on a circle about the axis through the scene camera's target along its up vector, each looking at the target"""
    cam = hs.camera
    up = cam["up"] / np.linalg.norm(cam["up"])
    arm = cam["eye"] - cam["target"]
    return [host.camera_pose_look_at(cam["look_at"], cam["target"] + rodrigues(np, up, 2.0 * math.pi * k / n) @ arm, cam["target"], cam["up"],
                                     aspect, cam["fov_deg"]) for k in range(n)]


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
        sys.exit("camera_pose_cost: no GPU (nothing is measured on a CPU)")
    W, H, spp, depth, n_tri = (480, 270, 8, 8, 3000) if a.small else (1920, 1080, 64, 8, 150000)
    raw = torch.zeros((H, W, 3), dtype=torch.float64, device="cuda:0")
    params = P.render_params(W, H, spp, depth)
    res = {"width": W, "height": H, "spp": spp, "max_bounces": depth, "repeats": a.repeats}

    # ---- the headline frame
    hs = host.shirley_spheres(W, H)
    oblique = (0.9 * np.array([0.3, -0.2, 0.5]), rodrigues(np, (0.3, 1.0, 2.0), 0.15))
    scenes = {k: P.Scene(hs.ptr, 0, keepalive=hs) for k in ("pose_off", "pose_identity", "pose_oblique")}
    scenes["pose_identity"].set_camera_pose(np.zeros(3), np.eye(3))
    scenes["pose_oblique"].set_camera_pose(*oblique)
    got = alternating_ms({k: (lambda g=g: g.render_raw_device(params, raw.data_ptr())) for k, g in scenes.items()}, a.repeats)
    for v in got.values():
        v["over_pose_off_ms"] = v["median_ms"] - got["pose_off"]["median_ms"]
    # the generator against its byte model
    timed = P.render_params(W, H, spp, depth, time_kernels=True)
    st = scenes["pose_oblique"].render_raw_device(timed, raw.data_ptr())
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
    copy_s = statistics.median(copy_runs[1:])
    traffic_rate = 2.0 * n_copy * 16 / copy_s  # bytes moved per second: every byte is read and written
    entries = spp * ((W + 7) // 8) * ((H + 7) // 8) * 64
    record_bytes = 48 + 32  # PtRayRec + PtPathRec (no emitter in this scene)
    res["headline"] = {"setups": got, "oblique_pose": {"origin": list(oblique[0]), "rotation": oblique[1].tolist()},
                       "pose_oblique_kernel_ms": st["kernel_ms"], "pose_oblique_kernel_launches": st["kernel_launches"],
                       "generator": {"entries": entries, "record_bytes": record_bytes, "measured_ms": st["kernel_ms"]["generate"],
                                     "float4_copy_bytes_per_s": traffic_rate,
                                     "byte_model_ms": entries * record_bytes / traffic_rate * 1e3}}
    for g in scenes.values():
        g.close()
    del src, dst

    # ---- the turntable
    hm = host.ganesha_like(W, H, n_tri)
    n_frames = 8
    poses = turntable_poses(np, host, hm, W / H, n_frames)
    one = P.Scene(hm.ptr, 0, keepalive=hm)

    def by_pose():
        for pose in poses:
            one.set_camera_pose(*pose)
            one.render_raw_device(params, raw.data_ptr())

    def by_rebuild(builder):
        def run():
            old = hm.d.reserved
            hm.d.reserved = builder  # 1 = the host BVH builder, 2 = the GPU one
            try:
                for _ in poses:
                    g = P.Scene(hm.ptr, 0, keepalive=hm)
                    g.render_raw_device(params, raw.data_ptr())
                    g.close()
            finally:
                hm.d.reserved = old
        return run
    tt = alternating_ms({"set_pose": by_pose, "rebuild_host_bvh": by_rebuild(1), "rebuild_gpu_bvh": by_rebuild(2)}, a.repeats)
    for v in tt.values():
        v["per_frame_ms"] = v["median_ms"] / n_frames
        v["over_set_pose"] = v["median_ms"] / tt["set_pose"]["median_ms"]
    res["turntable"] = {"frames": n_frames, "triangles": int(hm.d.n_triangles), "ways": tt}
    one.close()
    if headline:
        res["unposed_against_parent"] = headline
    text = json.dumps(res, indent=1)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
