"""The surface of ptx_walk_rays, checkable without a GPU: declared, exported and mirrored with no version touched, the walk constants
of include/ptx.h equal to the ctypes mirror's, and the refusals that need no device (the arguments are checked first)."""
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WALKS = ("SHARED_ASM", "OCT_ASM", "SHARED_DIV", "PACKET", "SHARED_ASM_ZERO", "OCT_ASM_ZERO", "SHARED_DIV_ZERO", "SHARED_ASM_TAIL",
         "OCT_ASM_TAIL", "SHARED_DIV_TAIL")


@pytest.fixture(scope="module")
def P():
    import path_tracer_ocaml_amd as P
    return P


def test_entry_point_and_constants_are_declared_exported_and_mirrored(P):
    header = open(os.path.join(ROOT, "include", "ptx.h")).read()
    assert re.search(r"\bptx_walk_rays\(", header)
    assert "ptx_walk_rays" in P.EXPORTS
    getattr(P.lib(), "ptx_walk_rays")
    values = []
    for name in WALKS:
        m = re.search(r"#define PTX_WALK_%s\s+(\d+)\b" % name, header)
        assert m, name
        assert getattr(P.abi, "PTX_WALK_" + name) == int(m.group(1)), name
        values.append(int(m.group(1)))
    assert sorted(values) == list(range(len(WALKS)))
    assert sorted(k for k in dir(P.abi) if k.startswith("PTX_WALK_")) == sorted("PTX_WALK_" + n for n in WALKS)
    assert P.lib().ptx_version() == 6  # an entry point only: no struct and no version changed


def test_refusals_that_need_no_device(P):
    from path_tracer_ocaml_amd import host
    hs = host.cornell_box(16, 16, 12.0)
    g = P.Scene(hs.ptr, -1, keepalive=hs)
    dp, ip = P.abi.c_double_p, P.abi.c_int32_p
    o, d, t, prim = np.zeros((4, 3)), np.tile([0.0, 0.0, -1.0], (4, 1)), np.full(4, -7.0), np.full(4, -7, dtype=np.int32)
    args = [o.ctypes.data_as(dp), d.ctypes.data_as(dp), t.ctypes.data_as(dp), prim.ctypes.data_as(ip)]
    L = P.lib()
    try:
        assert L.ptx_walk_rays(None, 0, 4, *args) == -1
        for k in range(4):
            assert L.ptx_walk_rays(g._h, 0, 4, *[None if j == k else a for j, a in enumerate(args)]) == -1
            assert "NULL" in P.last_error()
        for walk in (-1, len(WALKS), 1 << 20):
            assert L.ptx_walk_rays(g._h, walk, 4, *args) == -1
            assert "unknown walk" in P.last_error()
        for walk in range(len(WALKS)):  # a host-only scene: PTX_ERR_STATE, whatever the walk
            assert L.ptx_walk_rays(g._h, walk, 4, *args) == -3
            assert "host-only" in P.last_error()
            with pytest.raises(P.PtxError, match="host-only"):
                g.walk_rays(walk, o, d)
        assert (t == -7.0).all() and (prim == -7).all()  # nothing was written
    finally:
        g.close()
