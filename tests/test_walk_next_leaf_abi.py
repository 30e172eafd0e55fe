"""The surface of ptx_walk_next_leaf, checkable without a GPU: declared, exported and mirrored with no version touched, the walks it
takes named by ptx_walk_rays' constants, and the refusals that need no device (the arguments are checked first)."""
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TAKEN = ("SHARED_ASM", "OCT_ASM", "SHARED_DIV", "SHARED_ASM_ZERO", "OCT_ASM_ZERO", "SHARED_DIV_ZERO")
NOT_TAKEN = ("PACKET", "SHARED_ASM_TAIL", "OCT_ASM_TAIL", "SHARED_DIV_TAIL")


@pytest.fixture(scope="module")
def P():
    import path_tracer_ocaml_amd as P
    return P


def test_entry_point_is_declared_exported_and_mirrored(P):
    header = open(os.path.join(ROOT, "include", "ptx.h")).read()
    m = re.search(r"int32_t ptx_walk_next_leaf\(([^)]*)\)", header)
    assert m
    assert re.sub(r"\s+", " ", m.group(1)) == ("ptx_scene* scene, int32_t walk, int64_t n, const double* origins, const double* directions, "
                                               "const int32_t* nodes, const double* t_max, int32_t* leaf_out")
    assert "ptx_walk_next_leaf" in P.EXPORTS
    fn = getattr(P.lib(), "ptx_walk_next_leaf")
    assert len(fn.argtypes) == 8
    assert callable(P.Scene.walk_next_leaf)
    assert sorted(P.abi.PTX_NEXT_LEAF_WALKS) == sorted(getattr(P.abi, "PTX_WALK_" + n) for n in TAKEN)
    assert P.lib().ptx_version() == 6  # an entry point only: no struct and no version changed


def test_refusals_that_need_no_device(P):
    from path_tracer_ocaml_amd import host
    hs = host.cornell_box(16, 16, 12.0)
    g = P.Scene(hs.ptr, -1, keepalive=hs)
    dp, ip = P.abi.c_double_p, P.abi.c_int32_p
    o, d = np.zeros((4, 3)), np.tile([0.0, 0.0, -1.0], (4, 1))
    node, t_max, leaf = np.zeros(4, dtype=np.int32), np.full(4, 1.0), np.full(4, -7, dtype=np.int32)
    args = [o.ctypes.data_as(dp), d.ctypes.data_as(dp), node.ctypes.data_as(ip), t_max.ctypes.data_as(dp), leaf.ctypes.data_as(ip)]
    L = P.lib()
    try:
        assert L.ptx_walk_next_leaf(None, 0, 4, *args) == -1
        for k in range(5):
            assert L.ptx_walk_next_leaf(g._h, 0, 4, *[None if j == k else a for j, a in enumerate(args)]) == -1
            assert "NULL" in P.last_error()
        for walk in [-1, 10, 1 << 20] + [getattr(P.abi, "PTX_WALK_" + n) for n in NOT_TAKEN]:
            assert L.ptx_walk_next_leaf(g._h, walk, 4, *args) == -1
            assert "unknown walk" in P.last_error()
        for walk in P.abi.PTX_NEXT_LEAF_WALKS:  # a host-only scene: PTX_ERR_STATE, whatever the walk
            assert L.ptx_walk_next_leaf(g._h, walk, 4, *args) == -3
            assert "host-only" in P.last_error()
            with pytest.raises(P.PtxError, match="host-only"):
                g.walk_next_leaf(walk, o, d, node, t_max)
        with pytest.raises(ValueError):
            g.walk_next_leaf(0, o, d, node[:3], t_max)
        assert (leaf == -7).all()  # nothing was written
    finally:
        g.close()
