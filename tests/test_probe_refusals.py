"""What the point probes answer a call they refuse without touching a device (tests/probe_refusal_cases.py, host_cases): the return
code and the text of ptx_last_error, equal to tests/golden/probe_refusals.json -- recorded from the library before the probes moved
into csrc/probes.inc -- case by case, codes and texts alike."""
import pytest

import probe_refusal_cases as R


@pytest.fixture(scope="module")
def P():
    import path_tracer_ocaml_amd as P
    return P


def test_host_refusals_are_the_recorded_ones(P):
    scene = R.host_scene(P)
    try:
        got = R.run(P.lib(), R.host_cases(P, scene))
    finally:
        scene.close()
    want = R.golden("host")
    assert all(rc != 0 for _, rc, _ in got), [row for row in got if row[1] == 0]
    assert [row[0] for row in got] == [row[0] for row in want]  # the table is the recorded table
    assert got == want, [(g, w) for g, w in zip(got, want) if g != w][:5]


def test_the_table_covers_every_probe_and_every_required_pointer(P):
    """all fourteen exported probes; per probe the host-only scene (where it takes one), every pointer that must not be NULL, n = -1,
    and n = 2^31 - 1 where the count is bounded; the unknown walks; the two leaves' own ranges"""
    scene = R.host_scene(P)
    try:
        eps = R.entry_points(P, scene._h)
        labels = {row[0] for row in R.host_cases(P, scene)}
    finally:
        scene.close()
    assert len(eps) == 14 and all(name in P.EXPORTS for name in eps)
    for fn, args in eps.items():
        assert f"{fn}: n = -1" in labels
        assert (f"{fn}: n = 2^31 - 1" in labels) == (fn in R.BOUNDED)
        for name, kind, _ in args:
            assert (f"{fn}: {name} NULL" in labels) == (kind in ("scene", "ptr")), (fn, name)
    for w in (-1, 10, 1 << 20):
        assert f"ptx_walk_rays: walk {w}" in labels and f"ptx_walk_next_leaf: walk {w}" in labels
    for w in set(R.walks(P)) - set(P.abi.PTX_NEXT_LEAF_WALKS):
        assert f"ptx_walk_next_leaf: walk {w}" in labels
    assert {"ptx_math_eval: fn = 15", "ptx_lds_sample: dims[i] = dimension"} <= labels
    for what in ("a pose", "a shutter", "a lens", "the panorama"):
        assert f"ptx_debug_first_scatter: {what} on a host-only handle" in labels
