"""Run by tests/test_gpu_launch_args.py in a fresh process (PTX_BOUNCE_PACKET is read when a scene handle is created): on each
scene one small render, so that a queued bounce >= 1 has been launched on the handle, then the two calls that launch k_trace
outside the bounce loop -- ptx_intersect_rays on camera rays and ptx_render_features_device for the same frame.  Everything is
saved for the parent to compare.

usage: launch_args_gpu_child.py OUT.npz
"""
import os
import sys
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import exact_shading as S  # noqa: E402

W, H, SPP, DEPTH, N_RAYS = 32, 16, 2, 3, 256
SCENES = ("shirley", "cornell")  # Simd_leaf and Array_leaf, both LDS-resident
COUNTERS = ("segments", "nodes_tested", "prims_tested", "floor_tested")


def samples():
    """every pixel of every pass, pass-major: the first N_RAYS are pass 0 of the top rows"""
    ps, ys, xs = (a.ravel() for a in np.meshgrid(np.arange(SPP), np.arange(H), np.arange(W), indexing="ij"))
    return xs, ys, ps


def camera_rays(oracle, ptr, xs, ys, ps):
    """the oracle's camera rays of the samples at this depth (the sampler's table depends on it)"""
    cam = ptr.contents.camera
    tab = types.SimpleNamespace(cam4=np.array([cam.lower_left_x, cam.lower_left_y, cam.view_x, cam.view_y]))
    cx, cy, _ = S.camera_samples(tab, S.lds_alpha(oracle, 2 + 2 * DEPTH), W, H, SPP, xs, ys, ps, S.Decisions(len(xs)))
    return S.oracle_camera_rays(oracle, tab.cam4, cx, cy)


def main():
    import torch
    import path_tracer_ocaml_amd as P
    from oracle import oracle as O
    from path_tracer_ocaml_amd import abi
    O.lib()
    O.set_math(0)
    xs, ys, ps = samples()
    res = {}
    for name in SCENES:
        ptr, keep, _, _, _ = S.stock_desc(name, O, abi)
        g = P.Scene(ptr, 0, keepalive=keep)
        res[f"{name}/in_lds"] = np.array(int(g.stats()["traversal_in_lds"]))
        rgb, _ = g.render(W, H, SPP, DEPTH)
        res[f"{name}/rgb"] = rgb
        D = camera_rays(O, ptr, xs, ys, ps)[:N_RAYS]
        t, prim, st = g.intersect_rays(np.zeros_like(D), D)
        res[f"{name}/t"], res[f"{name}/prim"] = t, prim
        res[f"{name}/counters"] = np.array([st[k] for k in COUNTERS], dtype=np.int64)
        params = P.render_params(W, H, SPP, DEPTH)
        for first, count, key in [(0, SPP, "whole")] + [(p, 1, f"pass{p}") for p in range(SPP)]:
            f = torch.zeros((H, W, 8), dtype=torch.float64, device="cuda:0")
            g.render_features_device(params, first, count, f.data_ptr())
            res[f"{name}/feat/{key}"] = f.cpu().numpy()
        g.close()
    np.savez(sys.argv[1], **res)


if __name__ == "__main__":
    main()
