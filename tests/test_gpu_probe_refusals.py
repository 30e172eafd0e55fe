"""What the point probes answer a call they refuse on a scene that IS on a device (tests/probe_refusal_cases.py, gpu_cases): every
walk through ptx_walk_rays and ptx_walk_next_leaf on the scene of the wrong leaf kind, the _ZERO walks with an origin of -0.0, a node
index equal to the node count, a NaN t_max, an x = width and a pass = spp, the light half in emitted-only lighting, the environment
half with sampling off.  Codes and texts equal tests/golden/probe_refusals.json, recorded on an MI355X from the library before the
probes moved into csrc/probes.inc.  No refused call launches a kernel; after them each scene still walks 64 rays to the oracle's hits,
bit for bit."""
import ctypes as C

import numpy as np
import pytest

import probe_refusal_cases as R
from test_gpu_edge_cases import bits

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def P():
    import path_tracer_ocaml_amd as P
    assert P.lib().ptx_device_count() >= 1, P.last_error()
    return P


def test_device_refusals_are_the_recorded_ones_and_the_scenes_still_walk(P, oracle):
    (simd, d_simd, keep_simd), (array, d_array, keep_array) = R.gpu_scenes(P)
    try:
        assert simd.stats()["traversal_in_lds"] and array.stats()["traversal_in_lds"]
        got = R.run(P.lib(), R.gpu_cases(P, simd, array))
        want = R.golden("gpu")
        assert all(rc != 0 for _, rc, _ in got), [row for row in got if row[1] == 0]
        assert [row[0] for row in got] == [row[0] for row in want]
        assert got == want, [(g, w) for g, w in zip(got, want) if g != w][:5]
        # one accepted call each: the refusals left the handles as they were
        rng = np.random.default_rng(5)
        o = np.tile([0.0, 0.0, 2.0], (64, 1))
        d = np.array([0.0, 0.0, -4.0]) + rng.uniform(-1.0, 1.0, (64, 3)) - o
        for g, desc, keep, walk in ((simd, d_simd, keep_simd, P.abi.PTX_WALK_SHARED_ASM), (array, d_array, keep_array, P.abi.PTX_WALK_SHARED_DIV)):
            t_c, p_c, _ = oracle.Scene(C.pointer(desc), keep).intersect_rays(o, d)
            t_g, p_g = g.walk_rays(walk, o, d)
            assert (p_c >= 0).any()
            assert np.array_equal(p_g, p_c) and np.array_equal(bits(t_g), bits(t_c))
    finally:
        simd.close()
        array.close()
