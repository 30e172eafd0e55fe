"""Run by tests/test_gpu_lighting.py in a fresh process per schedule (the PTX_* variables are read when a scene handle is
created): ptx_trace_samples in lighting modes 1 and 2 for every scene and depth, saved for the parent to compare with the
restatement; with `--carry`, also which bounce kernel a frame of stock cornell took in modes 1, 2 and back in 0.

usage: lighting_gpu_child.py OUT.npz [--carry]
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import lighting_support as S  # noqa: E402

W, H, SPP, N = 96, 64, 16, 20000
DEPTHS = (1, 2, 8, 16)
SCENES = ("cornell", "lamp003", "mesh")


def descs(name):
    """(ptx_scene_desc or pointer, keepalive)"""
    from oracle import oracle as O
    if name == "cornell":
        d = O.desc_cornell(W, H)
        return d.ptr, d
    if name == "mesh":
        return S.mesh_with_lamp(O, W, H)
    hs = S.host_scene(name, W, H)
    return hs.ptr, hs


def samples():
    rng = np.random.default_rng(11)
    return rng.integers(0, W, N), rng.integers(0, H, N), rng.integers(0, SPP, N)


def main():
    import path_tracer_ocaml_amd as P
    out, carry = sys.argv[1], "--carry" in sys.argv[2:]
    xs, ys, ps = samples()
    res = {}
    for name in (("cornell",) if carry else SCENES):
        d, keep = descs(name)
        g = P.Scene(d, 0, keepalive=keep)
        res[f"{name}/in_lds"] = np.array(int(g.stats()["traversal_in_lds"]))
        for mode in (1, 2):
            g.set_lighting(mode)
            for depth in DEPTHS:
                rgb, st = g.trace_samples(W, H, SPP, depth, xs, ys, ps, count_work=True)
                res[f"{name}/{mode}/{depth}"] = rgb
                res[f"{name}/{mode}/{depth}/launches"] = np.array([st["carry_launches"], st["solo_launches"]])
            if carry:
                _, st = g.render(W, H, 4, 8, count_work=True)
                res[f"frame/{mode}"] = np.array([st["carry_launches"], st["solo_launches"]])
        if carry:
            g.set_lighting(0)
            _, st = g.render(W, H, 4, 8, count_work=True)
            res["frame/0"] = np.array([st["carry_launches"], st["solo_launches"]])
        g.close()
    np.savez(out, **res)


if __name__ == "__main__":
    main()
