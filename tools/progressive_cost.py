#!/usr/bin/env python3
"""What progressive rendering costs: ptx_render_progressive against ptx_render of the same frame, both into a pinned image,
alternated in one process.  passes_per_update K = 8, 16, 32 and N, with and without want_error; one JSON line per frame.
Usage: progressive_cost.py [reps] [frames...]  (frames: shirley_1080p, cornell_1024)"""
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402

import path_tracer_ocaml_amd as P  # noqa: E402
from path_tracer_ocaml_amd import host as H  # noqa: E402

FRAMES = {  # name: (scene builder, width, height, spp, depth) -- bench.py's headline frame and its cornell configuration
    "shirley_1080p": (lambda w, h: H.shirley_spheres(w, h), 1920, 1080, 64, 8),
    "cornell_1024": (lambda w, h: H.cornell_box(w, h), 1024, 1024, 256, 16),
}


def timed(fn):
    t0 = time.perf_counter()
    fn()
    return (time.perf_counter() - t0) * 1e3


def main():
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 5
    names = sys.argv[2:] or list(FRAMES)
    for name in names:
        build, w, h, spp, depth = FRAMES[name]
        hs = build(w, h)
        sc = P.Scene(hs.ptr, 0, keepalive=hs)
        img = np.zeros((h, w, 3))
        sc.pin_image(img)
        variants = [("render", None, None)]
        for k in (8, 16, 32, spp):
            for want in (False, True):
                variants.append((f"K{k}{'_err' if want else ''}", k, want))
        runs = {v[0]: [] for v in variants}
        updates = {}

        def run(v):
            label, k, want = v
            if k is None:
                return timed(lambda: sc.render(w, h, spp, depth, out=img))
            seen = []
            ms = timed(lambda: sc.render_progressive(w, h, spp, depth, k, want_error=want, out=img,
                                                     on_update=lambda *a: seen.append(a[0])))
            updates[label] = len(seen)
            return ms

        for v in variants:  # warm-up: workspaces, staging, first launches
            run(v)
        ref = None
        for _ in range(reps):
            for v in variants:  # alternated, so drift hits every variant alike
                runs[v[0]].append(run(v))
                if v[1] == spp and ref is not None:
                    assert np.array_equal(img.view(np.uint64), ref.view(np.uint64)), "the last update differs from ptx_render"
                if v[1] is None:
                    ref = img.copy()
        sc.unpin_image()
        base = statistics.median(runs["render"])
        out = {"frame": name, "width": w, "height": h, "spp": spp, "depth": depth, "reps": reps,
               "ptx_render_ms": round(base, 3),
               "progressive": {lab: {"ms": round(statistics.median(t), 3), "over_render": round(statistics.median(t) / base - 1, 4),
                                     "updates": updates.get(lab)} for lab, t in runs.items() if lab != "render"}}
        print(json.dumps(out), flush=True)
        sc.close()


if __name__ == "__main__":
    main()
