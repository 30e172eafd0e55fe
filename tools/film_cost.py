#!/usr/bin/env python3
"""What the film costs at other orders and radii.  Medians of 5 alternated runs after a warm-up, wall clock
around `--calls` back-to-back calls that each end in a device synchronise, divided by the number of calls.  Fails without a GPU.

At 1080p and 4K, spp 64, on seeded synthetic sums: ptx_film_resolve_device (k_film, the baseline) against
ptx_film_resolve_ex_device (k_film_wide) at (5, 1), (5, 0), (7, 3), (15, 7), with and without renormalisation, and the counts
pair on a mixed map.  The default film (5, 1) without renormalisation runs k_film whatever the entry point; PTX_FILM_WIDE=1 sends it
through k_film_wide for this comparison.
Each figure is reported in ms and as a share of the 21.7 ms headline frame.

usage: tools/film_cost.py [--out FILE.json] [--repeats 5] [--calls 10]"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
HEADLINE_MS = 21.7
FILMS = [(5, 1), (5, 0), (7, 3), (15, 7)]


def alternating_ms(fns, repeats, calls):
    """{name: (median, runs)} of several callables, one run of each in turn per round; a run is `calls` calls"""
    for f in fns.values():
        f()
    runs = {k: [] for k in fns}
    for _ in range(repeats):
        for k, f in fns.items():
            t0 = time.perf_counter()
            for _ in range(calls):
                f()
            runs[k].append((time.perf_counter() - t0) * 1e3 / calls)
    return {k: (statistics.median(v), v) for k, v in runs.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--spp", type=int, default=64)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--calls", type=int, default=10)
    a = ap.parse_args()
    import torch
    import path_tracer_ocaml_amd as P
    if P.lib().ptx_device_count() < 1:
        sys.exit("film_cost: no GPU (nothing is measured on a CPU)")
    res = {"spp": a.spp, "repeats": a.repeats, "calls_per_run": a.calls, "headline_ms": HEADLINE_MS, "sizes": {}}
    for name, (W, H) in (("1080p", (1920, 1080)), ("4k", (3840, 2160))):
        g = torch.Generator(device="cuda:0").manual_seed(1)
        raw = torch.rand((H, W, 3), dtype=torch.float64, device="cuda:0", generator=g) * a.spp
        counts = torch.randint(1, a.spp + 1, (H, W), dtype=torch.int32, device="cuda:0", generator=g)
        counts[: H // 2] = a.spp  # half the image agrees, half is mixed
        out = torch.zeros_like(raw)
        torch.cuda.synchronize()
        rp, cp, op = raw.data_ptr(), counts.data_ptr(), out.data_ptr()
        fns = {"k_film": lambda: P.film_resolve_device(0, W, H, a.spp, rp, op),
               "k_film_counts": lambda: P.film_resolve_counts_device(0, W, H, rp, cp, op)}
        for order, radius in FILMS:
            for renorm in (False, True):
                fns[f"ex_{order}_{radius}{'_renorm' if renorm else ''}"] = \
                    lambda film=(order, radius, renorm): P.film_resolve_device(0, W, H, a.spp, rp, op, film=film)
            fns[f"counts_ex_{order}_{radius}"] = lambda f=(order, radius): P.film_resolve_counts_device(0, W, H, rp, cp, op, film=f)
        os.environ["PTX_FILM_WIDE"] = "1"  # every ex_ call below runs k_film_wide, (5, 1) included; k_film / k_film_counts are ...
        plain = {k: fns.pop(k) for k in ("k_film", "k_film_counts")}

        def unforced(f):
            def run():
                os.environ["PTX_FILM_WIDE"] = "0"  # ... the scene-less entry points with the switch off
                f()
                os.environ["PTX_FILM_WIDE"] = "1"
            return run

        fns = {**{k: unforced(f) for k, f in plain.items()}, **fns}
        got = alternating_ms(fns, a.repeats, a.calls)
        del os.environ["PTX_FILM_WIDE"]
        res["sizes"][name] = {"width": W, "height": H,
                              "calls": {n: {"median_ms": m, "share_of_headline": m / HEADLINE_MS, "runs_ms": r}
                                        for n, (m, r) in got.items()}}
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
