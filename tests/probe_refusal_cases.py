"""Calls the point probes of include/ptx.h (csrc/probes.inc) must refuse, as one table, and a function that runs it.

The probes are the entry points that take n host-side items, launch one kernel over them and hand n results back: ptx_light_sample,
ptx_light_pdf, ptx_texture_eval, ptx_environment_eval / _sample / _pdf, ptx_trace_samples, ptx_camera_rays, ptx_intersect_rays,
ptx_walk_rays, ptx_walk_next_leaf, ptx_debug_first_scatter, ptx_lds_sample and ptx_math_eval (ptx_debug_filter_error, the fifteenth, is
compiled into diagnostic builds only and has no symbol in the product).  What a refused call answers -- the code and the text of
ptx_last_error -- is part of the ABI: tests/golden/probe_refusals.json holds what the library answered before the probes moved into a
file of their own, and tests/test_probe_refusals.py (`host`: no device is touched) and tests/test_gpu_probe_refusals.py (`gpu`: the
refusals that need a scene on a device) hold every later library to it.

A case is (label, entry point, arguments, changes, state): the entry point's baseline arguments -- valid ones, n = 4 -- with the
named ones replaced (None: a NULL pointer), called while `state` (None, or a pair of functions: set, undo) holds on the handle.

Recording (once, against the library the golden file is to pin, chosen with PTX_LIB):
    PTX_LIB=/path/to/libptx_hip.so python tests/probe_refusal_cases.py host|gpu [--out tests/golden/probe_refusals.json]"""
import ctypes as C
import json
import os
import sys

import numpy as np

N = 4
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "probe_refusals.json")
WIDTH, HEIGHT, SPP, DEPTH = 16, 8, 2, 4
BOUNDED = ("ptx_trace_samples", "ptx_camera_rays", "ptx_intersect_rays", "ptx_walk_rays", "ptx_walk_next_leaf")  # n < 2^31 - 1


def entry_points(P, handle, n=N):
    """entry point -> [(argument, kind, baseline value)] in include/ptx.h's order.  Kinds: scene, i32, i64, ptr (a NULL is refused)
    and opt (a NULL is accepted: an output the caller may leave out)"""
    def f(*shape):
        return np.zeros(shape)

    def i(*shape):
        return np.zeros(shape, dtype=np.int32)
    s, cnt = ("s", "scene", handle), ("n", "i64", n)

    def p():
        return ("p", "ptr", P.render_params(WIDTH, HEIGHT, samples_per_pixel=SPP, max_bounces=DEPTH))

    def triples():
        return [("xs", "ptr", i(n)), ("ys", "ptr", i(n)), ("passes", "ptr", i(n))]

    def rays():
        return [("origins", "ptr", f(n, 3)), ("directions", "ptr", np.tile([0.0, 0.0, -1.0], (n, 1)))]
    return {
        "ptx_light_sample": [s, cnt, ("points", "ptr", f(n, 3)), ("uv", "ptr", f(n, 2)), ("dir_out", "ptr", f(n, 3)), ("index_out", "opt", i(n))],
        "ptx_light_pdf": [s, cnt, ("points", "ptr", f(n, 3)), ("dirs", "ptr", f(n, 3)), ("pd_out", "ptr", f(n))],
        "ptx_texture_eval": [s, ("index", "i32", 0), cnt, ("uv", "ptr", f(n, 2)), ("rgb_out", "ptr", f(n, 3))],
        "ptx_environment_eval": [s, cnt, ("dirs", "ptr", f(n, 3)), ("rgb_out", "ptr", f(n, 3))],
        "ptx_environment_sample": [s, cnt, ("ab", "ptr", f(n, 2)), ("dirs_out", "ptr", f(n, 3)), ("texel_out", "opt", i(n, 2))],
        "ptx_environment_pdf": [s, cnt, ("dirs", "ptr", f(n, 3)), ("pd_out", "ptr", f(n))],
        "ptx_trace_samples": [s, p(), cnt] + triples() + [("rgb_out", "ptr", f(n, 3)), ("stats", "opt", P.abi.Stats())],
        "ptx_camera_rays": [s, p(), cnt] + triples() + [("origins_out", "ptr", f(n, 3)), ("directions_out", "ptr", f(n, 3))],
        "ptx_intersect_rays": [s, cnt] + rays() + [("t_out", "ptr", f(n)), ("prim_out", "ptr", i(n)), ("stats", "opt", P.abi.Stats())],
        "ptx_walk_rays": [s, ("walk", "i32", P.abi.PTX_WALK_SHARED_ASM), cnt] + rays() + [("t_out", "ptr", f(n)), ("prim_out", "ptr", i(n))],
        "ptx_walk_next_leaf": [s, ("walk", "i32", P.abi.PTX_WALK_SHARED_ASM), cnt] + rays()
                              + [("nodes", "ptr", i(n)), ("t_max", "ptr", f(n)), ("leaf_out", "ptr", i(n))],
        "ptx_debug_first_scatter": [s, p(), cnt] + triples() + [("ray_out", "ptr", f(n, 6)), ("attn_out", "ptr", f(n, 3)), ("alive_out", "ptr", i(n))],
        "ptx_lds_sample": [("device", "i32", 0), ("dimension", "i32", 4), cnt, ("offsets", "ptr", i(n)), ("dims", "ptr", i(n)), ("out", "ptr", f(n))],
        "ptx_math_eval": [("device", "i32", 0), ("fn", "i32", 0), cnt, ("a", "ptr", f(n)), ("b", "opt", f(n)), ("out", "ptr", f(n))],
    }


def walks(P):
    """PTX_WALK_* value -> name, the ten of them"""
    names = {getattr(P.abi, k): k for k in dir(P.abi) if k.startswith("PTX_WALK_")}
    assert sorted(names) == list(range(10))
    return names


def host_cases(P, scene):
    """the refusals no device is needed for, on a host-only scene (device -1) -- whose calls are all refused, in the order of each
    entry point's own checks: a NULL or a bad count may be answered before or after the scene's state, and that order is pinned too"""
    A, L = P.abi, P.lib()
    eps = entry_points(P, scene._h)
    cases = []
    for fn, args in eps.items():
        if args[0][1] == "scene":
            cases.append((fn + ": host-only scene", fn, args, {}, None))
        for name, kind, _ in args:
            if kind in ("scene", "ptr"):
                cases.append((f"{fn}: {name} NULL", fn, args, {name: None}, None))
        cases.append((fn + ": n = -1", fn, args, {"n": -1}, None))
        if fn in BOUNDED:
            cases.append((fn + ": n = 2^31 - 1", fn, args, {"n": 2 ** 31 - 1}, None))
    for fn in ("ptx_walk_rays", "ptx_walk_next_leaf"):
        unknown = [-1, 10, 1 << 20]
        if fn == "ptx_walk_next_leaf":  # the walks without a node loop of their own
            unknown += [A.PTX_WALK_PACKET, A.PTX_WALK_SHARED_ASM_TAIL, A.PTX_WALK_OCT_ASM_TAIL, A.PTX_WALK_SHARED_DIV_TAIL]
        for w in unknown:
            cases.append((f"{fn}: walk {w}", fn, eps[fn], {"walk": w}, None))
            cases.append((f"{fn}: walk {w}, NULL scene", fn, eps[fn], {"walk": w, "s": None}, None))
    cases.append(("ptx_math_eval: fn = 15", "ptx_math_eval", eps["ptx_math_eval"], {"fn": 15}, None))
    cases.append(("ptx_math_eval: fn = -1", "ptx_math_eval", eps["ptx_math_eval"], {"fn": -1}, None))
    dims = np.zeros(N, dtype=np.int32)
    dims[N - 1] = 4
    cases.append(("ptx_lds_sample: dims[i] = dimension", "ptx_lds_sample", eps["ptx_lds_sample"], {"dims": dims}, None))
    cases.append(("ptx_lds_sample: dimension = 0", "ptx_lds_sample", eps["ptx_lds_sample"], {"dimension": 0}, None))
    # ptx_debug_first_scatter answers for the camera's state before it looks at the device
    fs = "ptx_debug_first_scatter"
    eye, turn = np.zeros(3), np.eye(3).reshape(9)
    dp = A.c_double_p
    states = {
        "a pose": (lambda: L.ptx_scene_set_camera_pose(scene._h, eye.ctypes.data_as(dp), turn.ctypes.data_as(dp), None),
                   lambda: L.ptx_scene_set_camera_pose(scene._h, None, None, None)),
        "a shutter": (lambda: L.ptx_scene_set_camera_shutter(scene._h, np.array([0.1, 0.0, 0.0]).ctypes.data_as(dp),
                                                             np.array([0.0, 1.0, 0.0]).ctypes.data_as(dp), 0.0),
                      lambda: L.ptx_scene_set_camera_shutter(scene._h, None, None, 0.0)),
        "a lens": (lambda: L.ptx_scene_set_lens(scene._h, 0.05, 4.0), lambda: L.ptx_scene_set_lens(scene._h, 0.0, 4.0)),
        "the panorama": (lambda: L.ptx_scene_set_camera_projection(scene._h, A.PTX_PROJECTION_LATLONG),
                         lambda: L.ptx_scene_set_camera_projection(scene._h, A.PTX_PROJECTION_PERSPECTIVE)),
    }
    for what, state in states.items():
        cases.append((f"{fs}: {what} on a host-only handle", fs, eps[fs], {}, state))
    cases.append((fs + ": n = 0", fs, eps[fs], {"n": 0}, None))
    return cases


def gpu_scenes(P):
    """the two 60-sphere soups of tests/test_gpu_walk_rays.py's refusals, on device 0: (Simd_leaf, Array_leaf) as
    (P.Scene, descriptor, keepalive) each"""
    from test_gpu_edge_cases import make_desc
    from test_gpu_fuzz import sphere_soup
    out = []
    for leaf_kind in (0, 1):
        rng = np.random.default_rng(21)
        d, keep = make_desc(P.abi, spheres=sphere_soup(rng, 60, 1.0, np.array([0.0, 0.0, -4.0]), 4.0), leaf_kind=leaf_kind, cutoff=3)
        out.append((P.Scene(d, 0, keepalive=keep), d, keep))
    return out


def gpu_cases(P, simd, array):
    """the refusals that need a scene on a device (simd, array: P.Scene of a Simd_leaf and an Array_leaf scene held in LDS).  Every
    call is refused before anything is launched."""
    A = P.abi
    names = walks(P)
    scenes = {"Simd_leaf": (simd, entry_points(P, simd._h)), "Array_leaf": (array, entry_points(P, array._h))}
    minus_zero = np.zeros((N, 3))
    minus_zero[N - 1, 2] = -0.0
    cases = []
    for w, name in sorted(names.items()):
        short = name[len("PTX_WALK_"):]
        # the scene of the other leaf kind; the packet takes either, so nothing but its origin can be wrong
        wrong = ["Simd_leaf" if "DIV" in short else "Array_leaf"] if short != "PACKET" else ["Simd_leaf", "Array_leaf"]
        for kind in wrong:
            _, eps = scenes[kind]
            change = {"walk": w, "origins": minus_zero} if short == "PACKET" else {"walk": w}
            for fn in ("ptx_walk_rays", "ptx_walk_next_leaf"):
                cases.append((f"{fn}: {short} on the {kind} scene", fn, eps[fn], change, None))
        if short.endswith("_ZERO"):  # on the scene of its own kind, an origin of -0.0 in the last component
            kind = "Array_leaf" if "DIV" in short else "Simd_leaf"
            for fn in ("ptx_walk_rays", "ptx_walk_next_leaf"):
                cases.append((f"{fn}: {short} with an origin of -0.0", fn, scenes[kind][1][fn], {"walk": w, "origins": minus_zero}, None))
    for kind, w in (("Simd_leaf", A.PTX_WALK_SHARED_ASM), ("Array_leaf", A.PTX_WALK_SHARED_DIV)):
        scene, eps = scenes[kind]
        nodes = np.zeros(N, dtype=np.int32)
        nodes[N - 1] = scene.stats()["tree_nodes"]
        t_max = np.zeros(N)
        t_max[N - 1] = np.nan
        fn = "ptx_walk_next_leaf"
        cases.append((f"{fn}: node = the node count, {kind}", fn, eps[fn], {"walk": w, "nodes": nodes}, None))
        cases.append((f"{fn}: node = -1, {kind}", fn, eps[fn], {"walk": w, "nodes": np.full(N, -1, dtype=np.int32)}, None))
        cases.append((f"{fn}: t_max NaN, {kind}", fn, eps[fn], {"walk": w, "t_max": t_max}, None))
    _, eps = scenes["Simd_leaf"]
    xs, passes = np.zeros(N, dtype=np.int32), np.zeros(N, dtype=np.int32)
    xs[N - 1], passes[N - 1] = WIDTH, SPP
    for fn in ("ptx_trace_samples", "ptx_camera_rays"):
        cases.append((fn + ": x = width", fn, eps[fn], {"xs": xs}, None))
        cases.append((fn + ": pass = spp", fn, eps[fn], {"passes": passes}, None))
    cases.append(("ptx_light_sample: emitted-only lighting", "ptx_light_sample", eps["ptx_light_sample"], {}, None))
    cases.append(("ptx_light_pdf: emitted-only lighting", "ptx_light_pdf", eps["ptx_light_pdf"], {}, None))
    cases.append(("ptx_environment_sample: sampling off", "ptx_environment_sample", eps["ptx_environment_sample"], {}, None))
    cases.append(("ptx_environment_pdf: sampling off", "ptx_environment_pdf", eps["ptx_environment_pdf"], {}, None))
    cases.append(("ptx_texture_eval: index = the table's size", "ptx_texture_eval", eps["ptx_texture_eval"], {"index": 2}, None))
    return cases


def _c(kind, v):
    if v is None:
        return None
    if kind == "scene":
        return C.c_void_p(v)
    if kind in ("i32", "i64"):
        return (C.c_int32 if kind == "i32" else C.c_int64)(v)
    if isinstance(v, np.ndarray):
        assert v.flags["C_CONTIGUOUS"] and v.dtype in (np.float64, np.int32)
        return v.ctypes.data_as(C.POINTER(C.c_double if v.dtype == np.float64 else C.c_int32))
    return C.byref(v)


def run(L, cases):
    """every case called on the loaded library L -> [(label, return code, ptx_last_error's text)]"""
    L.ptx_last_error.restype = C.c_char_p
    out = []
    for label, fn, args, change, state in cases:
        assert set(change) <= {name for name, _, _ in args}, (label, change)
        if state:
            assert state[0]() == 0, label
        try:
            rc = getattr(L, fn)(*[_c(kind, change[name] if name in change else v) for name, kind, v in args])
            out.append((label, int(rc), (L.ptx_last_error() or b"").decode()))
        finally:
            if state:
                assert state[1]() == 0, label
    assert len({label for label, _, _ in out}) == len(out)
    return out


def host_scene(P):
    """a host-only scene (device -1): a few spheres, made without a device"""
    from test_gpu_edge_cases import make_desc
    spheres = [(float(x), 0.0, -5.0, 0.4, x % 3) for x in range(-2, 3)]
    d, keep = make_desc(P.abi, spheres=spheres, leaf_kind=0, cutoff=4)
    return P.Scene(d, -1, keepalive=keep)


def golden(half):
    return [tuple(row) for row in json.load(open(GOLDEN))[half]]


def main():
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import argparse
    ap = argparse.ArgumentParser()
    ap.add_argument("half", choices=("host", "gpu"))
    ap.add_argument("--out", default=GOLDEN)
    a = ap.parse_args()
    import path_tracer_ocaml_amd as P
    if a.half == "host":
        rows = run(P.lib(), host_cases(P, host_scene(P)))
    else:
        (simd, _, _), (array, _, _) = gpu_scenes(P)
        rows = run(P.lib(), gpu_cases(P, simd, array))
    not_refused = [r for r in rows if r[1] == 0]
    assert not not_refused, not_refused
    doc = json.load(open(a.out)) if os.path.exists(a.out) else {}
    doc[a.half] = rows
    with open(a.out, "w") as fh:
        json.dump(doc, fh, indent=1)
        fh.write("\n")
    print(f"{len(rows)} refusals recorded ({a.half}) -> {a.out}")


if __name__ == "__main__":
    main()
