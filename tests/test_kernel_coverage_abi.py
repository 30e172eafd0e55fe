"""The kernel table and the launch record, checkable without a GPU: ptx_kernel_table, ptx_scene_launched_kernels and
ptx_scene_clear_launched_kernels are declared, exported and mirrored with no version touched; the table has the instantiations the
selector comments of csrc/ptx_api.inc claim, under unique and stable names; the refusals that need no device; and the GPU case table of
test_gpu_kernel_coverage.py is complete -- its cases' expected sets and UNREACHABLE together are exactly the table, and disjoint."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# what the comments above the selectors say (k_bounce_carry: 24 + 6, k_bounce: 76 + 60)
COUNTS = {"k_trace": 32, "k_shade_pool": 12, "k_bounce_carry": 30, "k_bounce": 136}


@pytest.fixture(scope="module")
def P():
    import path_tracer_ocaml_amd as P
    return P


def family(name):
    return name.split("/")[0]


def test_entry_points_are_declared_exported_and_mirrored(P):
    header = open(os.path.join(ROOT, "include", "ptx.h")).read()
    for name in ("ptx_kernel_table", "ptx_scene_launched_kernels", "ptx_scene_clear_launched_kernels"):
        assert re.search(r"\b%s\(" % name, header)
        assert name in P.EXPORTS
        getattr(P.lib(), name)
    assert P.lib().ptx_version() == 6  # entry points only: no struct and no version changed
    assert P.abi.PTX_KERNEL_FAMILIES == tuple(COUNTS)


def test_the_table_has_what_the_selector_comments_claim(P):
    names = P.kernel_table()
    got = {f: sum(family(n) == f for n in names) for f in COUNTS}
    assert got == COUNTS and len(names) == sum(COUNTS.values())
    assert [family(n) for n in names] == [f for f in P.abi.PTX_KERNEL_FAMILIES for _ in range(COUNTS[f])]  # family by family
    text = open(os.path.join(ROOT, "path_tracer_ocaml_amd", "csrc", "ptx_api.inc")).read()
    for claim in ("k_trace: 32 =", "k_shade_pool: 12 =", "k_bounce_carry: 24 =", "+ 6 on the per-octant LDS image", "k_bounce: 76 =", "+ 60 with an image"):
        assert claim in text, claim
    assert P.lib().ptx_kernel_table(None, 0) == len(names)


def test_names_are_unique_and_stable(P):
    a, b = P.kernel_table(), P.kernel_table()
    assert a == b and len(set(a)) == len(a)
    assert all(re.fullmatch(r"k_[a-z_]+(/[a-z-]+)+", n) for n in a)
    assert "k_bounce/array/count/lit/queued/hbm/plain/img" in a


def test_refusals_that_need_no_device(P):
    from path_tracer_ocaml_amd import host
    L, ip = P.lib(), P.abi.c_int32_p
    need = sum(len(n) + 1 for n in P.kernel_table()) + 1
    buf = C.create_string_buffer(b"\x07" * need, need)
    for capacity in (-1, 0, 1, need - 1):  # a buffer too small: refused, nothing written
        assert L.ptx_kernel_table(buf, capacity) == -1
        assert "too small" in P.last_error() and buf.raw == b"\x07" * need
    assert L.ptx_kernel_table(buf, need) == len(P.kernel_table())
    assert buf.raw.endswith(b"\n\x00") and buf.value.decode().split("\n")[:-1] == P.kernel_table()
    idx = np.full(8, -7, dtype=np.int32)
    assert L.ptx_scene_launched_kernels(None, idx.ctypes.data_as(ip), 8) == -1
    assert "NULL scene" in P.last_error()
    assert L.ptx_scene_clear_launched_kernels(None) == -1
    assert "NULL scene" in P.last_error()
    hs = host.cornell_box(16, 16, 12.0)
    g = P.Scene(hs.ptr, -1, keepalive=hs)
    try:
        assert L.ptx_scene_launched_kernels(g._h, None, 8) == -1
        assert "NULL" in P.last_error()
        assert L.ptx_scene_launched_kernels(g._h, idx.ctypes.data_as(ip), -1) == -1
        assert "too small" in P.last_error()
        assert L.ptx_scene_launched_kernels(g._h, idx.ctypes.data_as(ip), 0) == 0  # a host-only scene has launched nothing
        assert g.launched_kernels() == []
        g.clear_launched_kernels()
        assert g.launched_kernels() == [] and (idx == -7).all()
    finally:
        g.close()


def test_the_gpu_case_table_is_complete(P):
    """from the table alone: every instantiation is expected by some case or listed as unreachable, never both, and nothing is
    expected that the library does not have"""
    import test_gpu_kernel_coverage as T
    table = set(P.kernel_table())
    unreachable = [name for name, _ in T.UNREACHABLE]
    assert len(set(unreachable)) == len(unreachable) and all(reason for _, reason in T.UNREACHABLE)
    reached = {}
    for case in T.CASES:
        want = T.expected(case)
        assert want and want <= table, (case.name, sorted(want - table))
        for name in want:
            reached.setdefault(name, case.name)
    assert not set(reached) & set(unreachable), sorted(set(reached) & set(unreachable))
    assert set(reached) | set(unreachable) == table, sorted(table - set(reached) - set(unreachable))
    assert 40 <= len(T.CASES) <= 70
    for case in T.CASES:  # the knobs are the ones the module knows, all of them set
        assert dict(case.knobs).keys() == T.KNOBS.keys(), case.name
