#!/usr/bin/env python3
"""What an image texture and an environment cost.  Medians of 5 alternated runs after a warm-up: wall clock around
one ptx_render_raw_device of the frame (it returns when the frame is complete), one run of each setup in turn per round.  Fails without
a GPU.

The headline frame (Shirley 1080p, spp 64, depth 8) under five setups:
  as_is            the scene as the benchmark renders it (shade-first order, per-octant LDS image, camera tile lists)
  checker_walk     the same checker with PTX_BOUNCE_ORDER=0 PTX_LDS_OCT=0 PTX_TILE_LISTS=0: the walk-first schedule an image scene takes,
                   without an image -- what of the difference below is the SCHEDULE
  image_nearest    the ground as a 1000 x 2000 image of the checker's two colours, nearest, repeat on both axes
  image_bilinear   the same, bilinear
  environment      a 2048 x 1024 environment, bilinear, in place of the sky
and the ganesha-like frame (150 k triangles on a floor, walked from HBM / L2) as it is and with a 500 x 500 image on its floor.
The image-against-checker difference is reported, not barred.

--parent-lib PATH: the headline against the parent commit.  PATH is libptx_hip.so built from the parent commit (a checkout of it
elsewhere, `make -C path_tracer_ocaml_amd/csrc`, the library copied to where this run can read it).  The tool then runs
`bench.py --gpus 1 --steps 3 --warmup 1 --no-workloads` as fresh child processes, `--repeats` times each, alternated, the parent's
runs with PTX_LIB=PATH (path_tracer_ocaml_amd loads that library instead of the tree's), BEFORE it touches the GPU itself; the scene
has no image, so the same device code must run.  Recorded beside the rest with the criterion: this median no worse than the parent's
median by more than (max - min) of the parent's own runs.

usage: tools/texture_cost.py [--out profiles/pr_image_textures_cost.json] [--repeats 5] [--parent-lib PATH] [--small]"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
WALK_FIRST = {"PTX_BOUNCE_ORDER": "0", "PTX_LDS_OCT": "0", "PTX_TILE_LISTS": "0"}


def alternating_ms(fns, repeats):
    """{name: (median, runs)} of several callables, one run of each in turn per round, after one warm-up of each"""
    for f in fns.values():
        f()
    runs = {k: [] for k in fns}
    for _ in range(repeats):
        for k, f in fns.items():
            t0 = time.perf_counter()
            f()
            runs[k].append((time.perf_counter() - t0) * 1e3)
    return {k: {"median_ms": statistics.median(v), "runs_ms": v} for k, v in runs.items()}


def scene_with_env(P, hs, env):
    """the knobs are read when the handle is created"""
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        return P.Scene(hs.ptr, 0, keepalive=hs)
    finally:
        for k, v in old.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v


def checker_image(np, w, h, even, odd):
    iy, ix = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    return np.where(((ix & 1) == (iy & 1))[:, :, None], np.asarray(even, dtype=np.float64), np.asarray(odd, dtype=np.float64))


def first_checker(desc):
    return next(i for i in range(desc.n_textures) if desc.textures[i].kind == 1)


BENCH = ["bench.py", "--gpus", "1", "--steps", "3", "--warmup", "1", "--no-workloads"]


def headline_against_parent(parent_lib, repeats):
    """alternated child processes of bench.py: the parent commit's library (PTX_LIB) and this tree's"""
    parent_lib = os.path.abspath(parent_lib)
    if not os.path.exists(parent_lib):
        sys.exit(f"texture_cost: {parent_lib} is missing")
    runs, unit = {"parent": [], "this": []}, None
    for _ in range(repeats):
        for which in ("parent", "this"):
            env = dict(os.environ)
            env.pop("PTX_LIB", None)
            if which == "parent":
                env["PTX_LIB"] = parent_lib
            r = subprocess.run([sys.executable] + BENCH, cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
            if r.returncode != 0:
                sys.exit(f"texture_cost: bench.py ({which}) failed: {r.stderr[-2000:]}")
            line = json.loads(r.stdout.strip().splitlines()[-1])
            runs[which].append(line["value"])
            unit = line.get("unit", "ms")
    pm, tm = statistics.median(runs["parent"]), statistics.median(runs["this"])
    spread = max(runs["parent"]) - min(runs["parent"])
    # a throughput (the benchmark's Msamples/s) must not fall below the parent's median by more than the spread, a time not rise above it
    ok = tm >= pm - spread if unit.endswith("/s") else tm <= pm + spread
    return {"command": "python " + " ".join(BENCH) + ", alternated parent (PTX_LIB) / this", "unit": unit, "runs": runs,
            "parent_median": pm, "this_median": tm, "parent_spread": spread, "within_parent_spread": ok}


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
        sys.exit("texture_cost: no GPU (nothing is measured on a CPU)")
    W, H, spp, depth, n_tri = (480, 270, 8, 8, 3000) if a.small else (1920, 1080, 64, 8, 150000)
    raw = torch.zeros((H, W, 3), dtype=torch.float64, device="cuda:0")
    params = P.render_params(W, H, spp, depth)
    res = {"width": W, "height": H, "spp": spp, "max_bounces": depth, "repeats": a.repeats, "frames": {}}

    def frame(g):
        return lambda: g.render_raw_device(params, raw.data_ptr())

    # ---- the headline frame
    hs = host.shirley_spheres(W, H)
    ground = first_checker(hs.ptr.contents)
    t = hs.ptr.contents.textures[ground]
    img = checker_image(np, 1000, 2000, list(t.even), list(t.odd))
    rng = np.random.default_rng(1)
    env = rng.uniform(0.0, 2.0, (1024, 2048, 3))
    scenes = {"as_is": P.Scene(hs.ptr, 0, keepalive=hs), "checker_walk": scene_with_env(P, hs, WALK_FIRST),
              "image_nearest": P.Scene(hs.ptr, 0, keepalive=hs), "image_bilinear": P.Scene(hs.ptr, 0, keepalive=hs),
              "environment": P.Scene(hs.ptr, 0, keepalive=hs)}
    scenes["image_nearest"].set_texture_image(ground, img, repeat=(True, True))
    scenes["image_bilinear"].set_texture_image(ground, img, bilinear=True, repeat=(True, True))
    scenes["environment"].set_environment(env)
    got = alternating_ms({k: frame(g) for k, g in scenes.items()}, a.repeats)
    base, walk = got["as_is"]["median_ms"], got["checker_walk"]["median_ms"]
    for k, v in got.items():
        v["over_as_is_ms"] = v["median_ms"] - base
        v["over_checker_walk_ms"] = v["median_ms"] - walk
    res["frames"]["shirley"] = {"setups": got, "schedule_share_of_nearest": (walk - base) / max(got["image_nearest"]["median_ms"] - base, 1e-9)}
    for g in scenes.values():
        g.close()
    # ---- the mesh frame
    hm = host.ganesha_like(W, H, n_tri)
    floor = hm.ptr.contents.materials[hm.ptr.contents.floor_material[0]].texture
    tf = hm.ptr.contents.textures[floor]
    fimg = checker_image(np, 500, 500, list(tf.even), list(tf.odd))
    scenes = {"as_is": P.Scene(hm.ptr, 0, keepalive=hm), "image_floor_nearest": P.Scene(hm.ptr, 0, keepalive=hm),
              "image_floor_bilinear": P.Scene(hm.ptr, 0, keepalive=hm)}
    scenes["image_floor_nearest"].set_texture_image(floor, fimg, repeat=(True, True))
    scenes["image_floor_bilinear"].set_texture_image(floor, fimg, bilinear=True, repeat=(True, True))
    got = alternating_ms({k: frame(g) for k, g in scenes.items()}, a.repeats)
    for k, v in got.items():
        v["over_as_is_ms"] = v["median_ms"] - got["as_is"]["median_ms"]
    res["frames"]["ganesha_like"] = {"triangles": n_tri, "setups": got}
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
