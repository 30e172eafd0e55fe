"""Run by tests/test_gpu_spherelight.py in a fresh process per schedule (the PTX_* variables are read when a scene handle is created):
ptx_trace_samples in lighting mode 2 with sphere light sampling on, for every scene of spherelight_support.SCENES and every depth, saved
for the parent to compare with the restatement.

usage: spherelight_gpu_child.py OUT.npz
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import spherelight_support as S  # noqa: E402


def main():
    import path_tracer_ocaml_amd as P
    from oracle import oracle as O
    O.lib()
    O.set_math(0)
    out = sys.argv[1]
    xs, ys, ps = S.samples()
    res = {}
    for name in S.SCENES:
        g = S.gpu_scene(P, name)
        res[f"{name}/in_lds"] = np.array(int(g.stats()["traversal_in_lds"]))
        res[f"{name}/lights"] = np.array([g.lighting()[1], g.sphere_lights()[1]])
        for depth in S.DEPTHS:
            rgb, st = g.trace_samples(S.W, S.H, S.SPP, depth, xs, ys, ps, count_work=True)
            res[f"{name}/{depth}"] = rgb
            res[f"{name}/{depth}/launches"] = np.array([st["carry_launches"], st["solo_launches"]])
        g.close()
    np.savez(out, **res)


if __name__ == "__main__":
    main()
