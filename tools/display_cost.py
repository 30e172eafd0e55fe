#!/usr/bin/env python3
"""What display outputs cost and save: medians of `--repeats` alternated runs on one MI355X after a warm-up, host
clock around calls that end in a device synchronise.  Fails without a GPU.

frame    the headline frame (Shirley, 1080p, spp 64, depth 8): the device-resident frame (ptx_render_raw_device plus the film);
         ptx_render into a pinned f64 image; ptx_render_display into a pinned RGB8, RGBA8 and RGB32F image; the unpinned forms.
         Each as a percentage over the device-resident frame, against the 3 % bar of a synchronous host-framebuffer call.
updates  ptx_render_progressive against ptx_render_progressive_display (RGBA8) at K = 8 and 64, with and without the error, and the
         denoised pair at K = 8, all into pinned images.
kernel   k_display_image alone per format at 1080p and 4K: device events around `--calls` calls; beside its byte model (24 bytes
         read and 3 / 4 / 12 / 16 written per pixel) at the rate a float4 copy of the same f64 image reaches in the same run.

usage: tools/display_cost.py [--out FILE.json] [--repeats 5] [--calls 20] [--parts frame,updates,kernel]"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
W, H, SPP, DEPTH = 1920, 1080, 64, 8
BAR = 0.03
LAYOUT = {"rgb8": ("uint8", 3), "rgba8": ("uint8", 4), "rgb32f": ("float32", 3), "rgba32f": ("float32", 4)}
SETTINGS = {"rgb8": ("reference", "none"), "rgba8": ("srgb", "aces"), "rgb32f": ("linear", "none"), "rgba32f": ("linear", "reinhard")}


def alternating_ms(fns, repeats):
    """{name: (median, runs)} of several callables, one run of each in turn per round, after one warm-up call of each"""
    for f in fns.values():
        f()
    runs = {k: [] for k in fns}
    for _ in range(repeats):
        for k, f in fns.items():
            t0 = time.perf_counter()
            f()
            runs[k].append((time.perf_counter() - t0) * 1e3)
    return {k: (statistics.median(v), v) for k, v in runs.items()}


def table(got, base=None):
    out = {}
    for k, (m, r) in got.items():
        out[k] = {"median_ms": round(m, 4), "runs_ms": [round(x, 4) for x in r]}
        if base is not None:
            out[k]["over_base"] = round(m / base - 1.0, 5)
    return out


def part_frame(P, Hh, np, torch, a):
    hs = Hh.shirley_spheres(W, H)
    scenes = []

    def scene():
        scenes.append(P.Scene(hs.ptr, 0, keepalive=hs))
        return scenes[-1]

    fns = {}
    dev = scene()
    params = P.render_params(W, H, SPP, DEPTH)
    d_raw = torch.zeros((H, W, 3), dtype=torch.float64, device="cuda:0")
    d_rgb = torch.zeros_like(d_raw)

    def device_resident():
        dev.render_raw_device(params, d_raw.data_ptr())
        P.film_resolve_device(0, W, H, SPP, d_raw.data_ptr(), d_rgb.data_ptr())

    fns["device_resident"] = device_resident
    for pinned in (True, False):
        tag = "pinned" if pinned else "unpinned"
        g, img = scene(), np.zeros((H, W, 3))
        if pinned:
            g.pin_image(img)
        fns[f"render_f64_{tag}"] = lambda g=g, img=img: g.render(W, H, SPP, DEPTH, out=img)
        for fmt in ("rgb8", "rgba8", "rgb32f"):
            dtype, ch = LAYOUT[fmt]
            g, out = scene(), np.zeros((H, W, ch), dtype=dtype)
            if pinned:
                g.image_pin_bytes(out)
            fns[f"render_display_{fmt}_{tag}"] = lambda g=g, out=out, fmt=fmt: g.render_display(
                W, H, SPP, DEPTH, format=fmt, transfer=SETTINGS[fmt][0], tone=SETTINGS[fmt][1], out=out)
    got = alternating_ms(fns, a.repeats)
    base = got["device_resident"][0]
    res = {"width": W, "height": H, "spp": SPP, "depth": DEPTH, "bar_over_device_resident": BAR, "calls": table(got, base)}
    res["rgba8_pinned_under_bar"] = bool(res["calls"]["render_display_rgba8_pinned"]["over_base"] <= BAR)
    for g in scenes:
        g.unpin_image()
        g.close()
    return res


def part_updates(P, Hh, np, torch, a):
    hs = Hh.shirley_spheres(W, H)
    scenes, fns = [], {}
    for k in (8, 64):
        for want in (False, True):
            tag = f"K{k}{'_err' if want else ''}"
            g, img = P.Scene(hs.ptr, 0, keepalive=hs), np.zeros((H, W, 3))
            g.pin_image(img)
            fns[f"progressive_f64_{tag}"] = lambda g=g, img=img, k=k, want=want: g.render_progressive(
                W, H, SPP, DEPTH, k, want_error=want, out=img)
            g2, out = P.Scene(hs.ptr, 0, keepalive=hs), np.zeros((H, W, 4), dtype=np.uint8)
            g2.image_pin_bytes(out)
            fns[f"progressive_rgba8_{tag}"] = lambda g=g2, out=out, k=k, want=want: g.render_progressive_display(
                W, H, SPP, DEPTH, k, format="rgba8", transfer="srgb", tone="aces", want_error=want, out=out)
            scenes += [g, g2]
    g, img = P.Scene(hs.ptr, 0, keepalive=hs), np.zeros((H, W, 3))
    g.pin_image(img)
    fns["denoised_f64_K8"] = lambda g=g, img=img: g.render_denoised(W, H, SPP, DEPTH, 8, out=img)
    g2, out = P.Scene(hs.ptr, 0, keepalive=hs), np.zeros((H, W, 4), dtype=np.uint8)
    g2.image_pin_bytes(out)
    fns["denoised_rgba8_K8"] = lambda g=g2, out=out: g.render_progressive_display(
        W, H, SPP, DEPTH, 8, denoise=True, format="rgba8", transfer="srgb", tone="aces", out=out)
    scenes += [g, g2]
    got = alternating_ms(fns, a.repeats)
    res = {"width": W, "height": H, "spp": SPP, "depth": DEPTH, "calls": table(got)}
    res["display_over_f64"] = {k.replace("_f64", ""): round(got[k.replace("_f64", "_rgba8")][0] / got[k][0] - 1.0, 5)
                               for k in got if "_f64" in k}
    for g in scenes:
        g.unpin_image()
        g.close()
    return res


def part_kernel(P, torch, a):
    res = {"calls_per_run": a.calls, "sizes": {}}
    for name, (w, h) in (("1080p", (1920, 1080)), ("4k", (3840, 2160))):
        n = w * h
        gen = torch.Generator(device="cuda:0").manual_seed(1)
        rgb = torch.rand((n, 3), dtype=torch.float64, device="cuda:0", generator=gen) * 1.2
        copy_dst = torch.zeros_like(rgb)
        outs = {fmt: torch.zeros(n * P.display_pixel_bytes(fmt), dtype=torch.uint8, device="cuda:0") for fmt in LAYOUT}
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

        def events(f):
            torch.cuda.synchronize()
            start.record()
            for _ in range(a.calls):
                f()
            stop.record()
            stop.synchronize()
            return start.elapsed_time(stop) / a.calls

        fns = {"float4_copy": lambda: copy_dst.view(torch.float32).view(-1, 4).copy_(rgb.view(torch.float32).view(-1, 4))}
        for fmt in LAYOUT:
            fns[fmt] = lambda fmt=fmt: P.display_image_device(0, n, rgb.data_ptr(), outs[fmt].data_ptr(), format=fmt,
                                                              transfer=SETTINGS[fmt][0], tone=SETTINGS[fmt][1])
        for f in fns.values():
            f()
        runs = {k: [] for k in fns}
        for _ in range(a.repeats):
            for k, f in fns.items():
                runs[k].append(events(f))
        med = {k: statistics.median(v) for k, v in runs.items()}
        rate = 2 * n * 24 / (med["float4_copy"] * 1e-3)  # bytes read + written per second
        size = {"width": w, "height": h, "float4_copy_ms": round(med["float4_copy"], 5), "float4_copy_GBps": round(rate / 1e9, 1), "formats": {}}
        for fmt in LAYOUT:
            model = n * (24 + P.display_pixel_bytes(fmt))
            size["formats"][fmt] = {"transfer": SETTINGS[fmt][0], "tone": SETTINGS[fmt][1], "median_ms": round(med[fmt], 5),
                                    "runs_ms": [round(x, 5) for x in runs[fmt]], "model_bytes": model,
                                    "model_ms_at_copy_rate": round(model / rate * 1e3, 5),
                                    "over_model": round(med[fmt] / (model / rate * 1e3) - 1.0, 4)}
        res["sizes"][name] = size
    res["note"] = ("the per-call figure includes ptx_display_image_device's wait for the stream after every launch: the host's "
                   "launch-and-wait round trip, not the kernel alone, bounds it from below")
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--parts", default="frame,updates,kernel")
    a = ap.parse_args()
    import numpy as np
    import torch
    import path_tracer_ocaml_amd as P
    from path_tracer_ocaml_amd import host as Hh
    if P.lib().ptx_device_count() < 1:
        sys.exit("display_cost: no GPU (nothing is measured on a CPU)")
    res = {"repeats": a.repeats}
    for part in a.parts.split(","):
        if part == "frame":
            res["frame"] = part_frame(P, Hh, np, torch, a)
        elif part == "updates":
            res["updates"] = part_updates(P, Hh, np, torch, a)
        elif part == "kernel":
            res["kernel"] = part_kernel(P, torch, a)
        else:
            sys.exit(f"display_cost: unknown part {part!r}")
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
