#!/usr/bin/env python3
"""What cone-sampling emissive spheres costs and buys.  Medians of `--repeats` alternated runs after a warm-up;
fails without a GPU.

The headline scene (Shirley, 1080p, spp 64, depth 8) with a lamp sphere hung into it (`--sphere-lamp`: world X,Y,Z,R,EMIT, default
0,4,0,0.5,40) in three setups of one scene handle, alternated: `reference` (mode 0), `path-order` (mode 1) and `sampled` (mode 2 with
ptx_scene_set_sphere_light_sampling).  Per setup: ms per frame (wall clock around one ptx_render_raw_device, which returns when the
frame is complete), and from one ptx_render_progressive run's error image the per-pixel standard error (mean of r, g, b) -- its median
over the pixels and the frame's root mean square -- and the time the setup would need to reach `sampled`'s rms error, standard error
falling as 1 / sqrt(passes).

--parent-lib PATH: an existing lit case with the option OFF against the parent commit, whose LIT kernels did not carry the sphere arm:
cornell 1024 x 1024, spp 64, depth 8, with the lamp of --lamp=0.03,0.999,400, mode 2.  PATH is libptx_hip.so built from the parent
commit.  The tool runs itself as fresh child processes (`--child-cornell`), `--repeats` times each, alternated, the parent's runs with
PTX_LIB=PATH, BEFORE it touches the GPU itself, and then the same A/B once more parent against parent: the spread of that run is what
the difference is read against.

usage: tools/sphere_light_cost.py [--out profiles/pr_sphere_lights_cost.json] [--repeats 5] [--parent-lib PATH] [--small]
                                  [--sphere-lamp X,Y,Z,R,EMIT]"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)


def cornell_child(small):
    """one JSON line: the median of 3 frames of the lit case after a warm-up"""
    import torch
    import path_tracer_ocaml_amd as P
    from path_tracer_ocaml_amd import host
    w = h = 256 if small else 1024
    spp, depth = (8, 8) if small else (64, 8)
    hs = host.cornell_lamp(w, h, 0.0, 0.03, 0.999, 400.0)
    g = P.Scene(hs.ptr, 0, keepalive=hs)
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
        sys.exit(f"sphere_light_cost: {parent_lib} is missing")
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
                    sys.exit(f"sphere_light_cost: the child ({which}) failed: {r.stderr[-2000:]}")
                line = json.loads(r.stdout.strip().splitlines()[-1])
                runs[which].append(line["median_ms"])
                sums[which] = line["checksum"]
        return runs, sums

    runs, sums = ab({"parent": parent_lib, "this": None})
    same, _ = ab({"parent_a": parent_lib, "parent_b": parent_lib})
    pm, tm = statistics.median(runs["parent"]), statistics.median(runs["this"])
    spread = abs(statistics.median(same["parent_a"]) - statistics.median(same["parent_b"]))
    return {"case": "cornell with the lamp 0.03,0.999,400 (ceiling black), mode 2, sphere light sampling off", "runs_ms": runs,
            "parent_median_ms": pm, "this_median_ms": tm, "this_over_parent": tm / pm - 1.0, "parent_to_parent_runs_ms": same,
            "parent_to_parent_median_difference_ms": spread, "moves_more_than_parent_to_parent": abs(tm - pm) > spread,
            "same_frame": sums["parent"] == sums["this"]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--parent-lib", default=None, help="libptx_hip.so built from the parent commit: also run the lit-case A/B")
    ap.add_argument("--small", action="store_true", help="a 480 x 270 frame, spp 8: checks the tool, measures nothing")
    ap.add_argument("--sphere-lamp", default="0,4,0,0.5,40", help="world X,Y,Z,R,EMIT of the lamp sphere")
    ap.add_argument("--child-cornell", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child_cornell:
        return cornell_child(a.small)
    lamp = [float(v) for v in a.sphere_lamp.split(",")]
    if len(lamp) != 5:
        sys.exit("sphere_light_cost: --sphere-lamp takes X,Y,Z,R,EMIT")
    lit = cornell_against_parent(a.parent_lib, a.repeats, a.small) if a.parent_lib else None  # child processes first: no GPU open here yet
    import numpy as np
    import torch
    import path_tracer_ocaml_amd as P
    from path_tracer_ocaml_amd import host
    if P.lib().ptx_device_count() < 1:
        sys.exit("sphere_light_cost: no GPU (nothing is measured on a CPU)")
    W, H, spp, depth = (480, 270, 8, 8) if a.small else (1920, 1080, 64, 8)
    hs = host.shirley_lamp(W, H, lamp)
    g = P.Scene(hs.ptr, 0, keepalive=hs)
    g.set_sphere_light_sampling(True)
    raw = torch.zeros((H, W, 3), dtype=torch.float64, device="cuda:0")
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
    res = {"scene": "shirley with --sphere-lamp=" + a.sphere_lamp, "width": W, "height": H, "spp": spp, "max_bounces": depth,
           "repeats": a.repeats, "setups": {}}
    err = {}
    for k, mode in setups.items():
        g.set_lighting(mode)
        _, e, done, _ = g.render_progressive(W, H, spp, depth, spp, want_error=True)
        assert done == spp
        e = e.mean(axis=2)
        err[k] = {"median": float(np.median(e)), "rms": float(np.sqrt((e * e).mean())), "zero_share": float((e == 0.0).mean())}
    for k in setups:
        ms = statistics.median(runs[k])
        e, t = err[k], err["sampled"]
        res["setups"][k] = {
            "median_ms": ms, "runs_ms": runs[k], "over_reference": ms / statistics.median(runs["reference"]) - 1.0,
            "median_pixel_stderr": e["median"], "rms_pixel_stderr": e["rms"], "pixels_with_zero_error": e["zero_share"],
            "ms_to_sampled_rms_error": ms * (e["rms"] / t["rms"]) ** 2 if t["rms"] > 0.0 else None,
        }
    g.close()
    if lit:
        res["lit_case_against_parent"] = lit
    text = json.dumps(res, indent=1)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
