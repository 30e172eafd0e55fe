"""The GPU BVH builder (csrc/bvh_build_gpu.inc) on the degenerate inputs of tests/bvh_families.py: the tree it leaves is
the host builder's bit for bit -- boxes as u64, node info, leaf element order, node / depth / leaf / slot counts -- with no
tolerance anywhere.  tests/test_bvh_families.py ties the host-only scene of the same descriptors to the oracle, so nothing
here needs the oracle except the tests of which builder a descriptor gets.  No ray is traced through these trees: equal
trees give equal host arrays, and the walks have adversarial tests of their own (test_gpu_walk_rays.py).

Every device build is preceded by the depth condition of bvh_families.MAX_DEPTH on the host-built tree."""
import ctypes as C
import time

import numpy as np
import pytest

import bvh_families as F

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def P():
    import path_tracer_ocaml_amd as P
    assert P.lib().ptx_device_count() >= 1, P.last_error()
    t0 = time.perf_counter()
    yield P
    print(f"test_gpu_bvh_families: {time.perf_counter() - t0:.2f} s for the module")


_host = {}


def host_tree(P, name):
    """(desc, keepalive, tree, stats) of a family's host-only scene, built once; refuses a tree deeper than MAX_DEPTH"""
    if name not in _host:
        d, keep = F.FAMILIES[name]()
        h = P.Scene(d, -1, keepalive=keep)
        _host[name] = (d, keep, h.tree(), h.stats())
        h.close()
    d, keep, tree, stats = _host[name]
    assert not stats["bvh_built_on_gpu"]
    assert stats["tree_depth"] <= F.MAX_DEPTH, f"{name}: depth {stats['tree_depth']} is not taken to a device"
    return d, keep, tree, stats


def with_builder(d, reserved):
    from path_tracer_ocaml_amd import abi
    c = abi.SceneDesc()
    C.memmove(C.byref(c), C.byref(d), C.sizeof(c))
    c.reserved = reserved
    return c


def device_scene_equals_host(P, name, reserved, on_gpu):
    d, keep, tree, stats = host_tree(P, name)  # asserts the depth first
    g = P.Scene(with_builder(d, reserved), 0, keepalive=keep)
    try:
        gs = g.stats()
        assert gs["bvh_built_on_gpu"] == on_gpu
        assert F.same_tree(g.tree(), tree) == [], name
        assert [gs[k] for k in F.STAT_KEYS] == [stats[k] for k in F.STAT_KEYS]
    finally:
        g.close()


def refused(P, name, reserved, device, match):
    d, keep, _, _ = host_tree(P, name)
    with pytest.raises(P.PtxError, match=match) as e:
        P.Scene(with_builder(d, reserved), device, keepalive=keep)
    assert "GPU BVH build failed" not in str(e.value)  # an argument error with its reason, not a HIP error string
    device_scene_equals_host(P, "soup-65", 2, True)  # the next ordinary scene still builds
    device_scene_equals_host(P, "soup-8193", 0, True)


@pytest.mark.parametrize("name", F.GPU_FAMILIES)
def test_gpu_builder_equals_host_builder(P, name):
    device_scene_equals_host(P, name, 2, True)


# ---------------------------------------------------------------- which builder a descriptor gets
def test_automatic_choice_flips_at_4096(P, oracle):
    for n, on_gpu in ((4095, False), (4096, True)):
        d, keep, tree, _ = host_tree(P, f"soup-{n}")
        o = oracle.Scene(C.pointer(d), keep)
        assert F.same_tree(tree, o.tree()) == []
        o.close()
        device_scene_equals_host(P, f"soup-{n}", 0, on_gpu)


def test_more_bins_than_the_gpu_builder_has(P, oracle):
    d, keep, tree, _ = host_tree(P, "soup-9000-bins65")
    o = oracle.Scene(C.pointer(d), keep)
    assert F.same_tree(tree, o.tree()) == []
    o.close()
    device_scene_equals_host(P, "soup-9000-bins65", 0, False)
    refused(P, "soup-9000-bins65", 2, 0, "num_bins > 64")


def test_gpu_builder_for_a_host_only_scene_is_refused(P):
    refused(P, "soup-8193", 2, -1, "host-only scene")


# ---------------------------------------------------------------- signed zeros
@pytest.mark.parametrize("name", [n for n, why in F.GPU_REFUSED.items() if why == "zero"])
def test_bound_columns_with_both_zeros_go_to_the_host_builder(P, name):
    """The GPU builder reduces bounds with integer min / max over order-preserving images, where -0.0 < +0.0; the host
    builder and the oracle keep whichever zero Float.min / Float.max meet second.  A column that holds both zeros is
    therefore left to the host builder (DESIGN F3): silently when the choice is automatic, with an argument error when
    the GPU builder was asked for.  (signed-zero-negative, one zero per column, is among the GPU families above.)"""
    device_scene_equals_host(P, name, 0, False)
    refused(P, name, 2, 0, r"\+0\.0 and -0\.0")


# ---------------------------------------------------------------- one workspace, many builds
def test_workspace_reuse_across_sizes(P):
    """The builder's buffers belong to the thread and only grow; the counters and the work lists carry the last build's
    contents.  Large, tiny (one wave, nothing tiled), one 9000-element leaf (a tiled segment that does not split), just
    above the tile threshold, large again: each tree is its host tree."""
    for name in ("soup-20000", "soup-5", "coincident-9000", "soup-8193", "soup-20000"):
        device_scene_equals_host(P, name, 2, True)
