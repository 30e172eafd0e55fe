#!/usr/bin/env python3
"""What importance-sampling the environment costs and buys.  Medians of `--repeats` alternated runs after a
warm-up; fails without a GPU.

The headline scene (Shirley, 1080p, spp 64, depth 8) under a 2048 x 1024 environment -- a dim sky with a sun of 3 x 3 texels, bilinear
-- in three setups of one scene handle, alternated: `reference` (mode 0), `path-order` (mode 1) and `sampled` (mode 2 with
ptx_scene_set_environment_sampling).  Per setup: ms per frame (wall clock around one ptx_render_raw_device, which returns when the
frame is complete), the per-pixel standard error e = sqrt(se_r^2 + se_g^2 + se_b^2) from the square sums of one
ptx_render_passes_device frame -- its median over the pixels, the share of pixels with e = 0 and the frame's root mean square -- and
the time the setup would need to reach `sampled`'s figure, standard error falling as 1 / sqrt(passes), for the median and for the rms.

--parent-lib PATH: the existing lit-and-image case against the parent commit, whose 22 LIT && IMG kernels did not carry the new arm:
cornell 1024 x 1024, spp 64, depth 8, with a 512 x 512 image on the floor's texture entry, mode 2, sampling off.  PATH is libptx_hip.so
built from the parent commit.  The tool runs itself as fresh child processes (`--child-cornell`), `--repeats` times each, alternated,
the parent's runs with PTX_LIB=PATH, BEFORE it touches the GPU itself, and then the same A/B once more parent against parent: the
spread of that run is what the difference is read against.

usage: tools/env_sampling_cost.py [--out profiles/pr_env_sampling_cost.json] [--repeats 5] [--parent-lib PATH] [--small]"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)


def sun_sky(np, width, height):
    rng = np.random.default_rng(2)
    img = rng.uniform(0.05, 0.15, (height, width, 3))
    cx, cy = (width * 5) // 8, (height * 11) // 16  # row 0 is straight down: the sun stands about 34 degrees above the horizon
    img[cy - 1:cy + 2, cx - 1:cx + 2] = [60000.0, 55000.0, 50000.0]
    return img


def cornell_child(small):
    """one JSON line: the median of 3 frames of the lit-and-image case after a warm-up"""
    import numpy as np
    import torch
    import path_tracer_ocaml_amd as P
    from path_tracer_ocaml_amd import host
    w = h = 256 if small else 1024
    spp, depth = (8, 8) if small else (64, 8)
    hs = host.cornell_box(w, h, 12.0)
    g = P.Scene(hs.ptr, 0, keepalive=hs)
    rng = np.random.default_rng(3)
    g.set_texture_image(4, rng.uniform(0.05, 0.95, (512, 512, 3)), bilinear=True, repeat=(False, True))  # the floor's entry
    g.set_lighting("sampled")
    raw = torch.zeros((h, w, 3), dtype=torch.float64, device="cuda:0")
    params = P.render_params(w, h, spp, depth)
    g.render_raw_device(params, raw.data_ptr())
    runs = []
    for _ in range(3):
        t0 = time.perf_counter()
        g.render_raw_device(params, raw.data_ptr())
        runs.append((time.perf_counter() - t0) * 1e3)
    print(json.dumps({"median_ms": statistics.median(runs), "runs_ms": runs, "checksum": float(raw.sum().item())}))
    g.close()


def cornell_against_parent(parent_lib, repeats, small):
    parent_lib = os.path.abspath(parent_lib)
    if not os.path.exists(parent_lib):
        sys.exit(f"env_sampling_cost: {parent_lib} is missing")
    cmd = [sys.executable, os.path.abspath(__file__), "--child-cornell"] + (["--small"] if small else [])

    def ab(libs):
        runs, sums = {k: [] for k in libs}, {}
        for _ in range(repeats):
            for which, lib in libs.items():
                env = dict(os.environ)
                env.pop("PTX_LIB", None)
                if lib:
                    env["PTX_LIB"] = lib
                r = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
                if r.returncode != 0:
                    sys.exit(f"env_sampling_cost: the child ({which}) failed: {r.stderr[-2000:]}")
                line = json.loads(r.stdout.strip().splitlines()[-1])
                runs[which].append(line["median_ms"])
                sums[which] = line["checksum"]
        return runs, sums

    runs, sums = ab({"parent": parent_lib, "this": None})
    same, _ = ab({"parent_a": parent_lib, "parent_b": parent_lib})
    pm, tm = statistics.median(runs["parent"]), statistics.median(runs["this"])
    spread = abs(statistics.median(same["parent_a"]) - statistics.median(same["parent_b"]))
    return {"case": "cornell with a 512 x 512 bilinear image on the floor, mode 2, sampling off", "runs_ms": runs, "parent_median_ms": pm,
            "this_median_ms": tm, "this_over_parent": tm / pm - 1.0, "parent_to_parent_runs_ms": same,
            "parent_to_parent_median_difference_ms": spread, "moves_more_than_parent_to_parent": abs(tm - pm) > spread,
            "same_frame": sums["parent"] == sums["this"]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--parent-lib", default=None, help="libptx_hip.so built from the parent commit: also run the lit-and-image A/B")
    ap.add_argument("--small", action="store_true", help="a 480 x 270 frame, spp 8: checks the tool, measures nothing")
    ap.add_argument("--child-cornell", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child_cornell:
        return cornell_child(a.small)
    lit = cornell_against_parent(a.parent_lib, a.repeats, a.small) if a.parent_lib else None  # child processes first: no GPU open here yet
    import numpy as np
    import torch
    import path_tracer_ocaml_amd as P
    from path_tracer_ocaml_amd import host
    if P.lib().ptx_device_count() < 1:
        sys.exit("env_sampling_cost: no GPU (nothing is measured on a CPU)")
    W, H, spp, depth = (480, 270, 8, 8) if a.small else (1920, 1080, 64, 8)
    hs = host.shirley_spheres(W, H)
    g = P.Scene(hs.ptr, 0, keepalive=hs)
    t = np.deg2rad(30.0)  # about the camera-space y axis
    g.set_environment(sun_sky(np, 2048, 1024), [[np.cos(t), 0.0, np.sin(t)], [0.0, 1.0, 0.0], [-np.sin(t), 0.0, np.cos(t)]])
    g.set_environment_sampling(True)
    raw = torch.zeros((H, W, 3), dtype=torch.float64, device="cuda:0")
    sq = torch.zeros_like(raw)
    params = P.render_params(W, H, spp, depth)
    setups = {"reference": 0, "path-order": 1, "sampled": 2}

    def frame(mode):
        g.set_lighting(mode)
        g.render_raw_device(params, raw.data_ptr())

    for mode in setups.values():
        frame(mode)
    runs = {k: [] for k in setups}
    for _ in range(a.repeats):
        for k, mode in setups.items():
            t0 = time.perf_counter()
            frame(mode)
            runs[k].append((time.perf_counter() - t0) * 1e3)
    res = {"scene": "shirley under a 2048 x 1024 bilinear sun sky (3 x 3 texels)", "width": W, "height": H, "spp": spp, "max_bounces": depth,
           "repeats": a.repeats, "setups": {}}
    err = {}
    for k, mode in setups.items():
        g.set_lighting(mode)
        raw.zero_()
        sq.zero_()
        g.render_passes_device(params, 0, spp, raw.data_ptr(), sq.data_ptr())
        se2 = torch.clamp(sq - raw * raw / spp, min=0.0) / (spp * (spp - 1.0))
        e = torch.sqrt(se2.sum(dim=2)).flatten()
        err[k] = {"median": float(e.median().item()), "rms": float(torch.sqrt((e * e).mean()).item()), "zero_share": float((e == 0).double().mean().item())}
    for k in setups:
        ms = statistics.median(runs[k])
        e, t = err[k], err["sampled"]
        res["setups"][k] = {
            "median_ms": ms, "runs_ms": runs[k], "over_reference": ms / statistics.median(runs["reference"]) - 1.0,
            "median_pixel_stderr": e["median"], "rms_pixel_stderr": e["rms"], "pixels_with_zero_error": e["zero_share"],
            "ms_to_sampled_median_error": ms * (e["median"] / t["median"]) ** 2 if t["median"] > 0.0 else None,
            "ms_to_sampled_rms_error": ms * (e["rms"] / t["rms"]) ** 2 if t["rms"] > 0.0 else None,
        }
    g.close()
    if lit:
        res["lit_and_image_against_parent"] = lit
    text = json.dumps(res, indent=1)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
