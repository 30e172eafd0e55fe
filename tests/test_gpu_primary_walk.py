"""The two walks of the camera rays on LDS-resident scenes (PTX_PRIMARY_WALK, read when the scene handle is created):

  0            pt_trace_packet: the 64 rays of an 8 x 8 tile walk the tree together, one shared stack of (node, lane mask)
  1            pt_trace_ray: one ray per lane, the walk of the queued rays (Simd_leaf, not counting: the assembly node loop;
               counting: the C++ loop), without a tail cut
  2 (default)  by scene: 1 for Simd_leaf scenes, 0 for Array_leaf scenes

A ray's own sequence of box and packet tests is the same in both, so the raw per-pixel sums are bit-identical between the two and
to the CPU oracle and every work counter is equal.  ptx_stats.primary_lane_walks (counting renders) says which walk ran: one count
per camera launch that walked per lane.

The images are the smallest at which the walks differ in what they do: 13 x 11 has one ragged tile row and column (lanes without
a sample walk a dummy ray and must stay out of results and counters), 72 x 40 has the image centre inside a tile (mixed direction
signs in one wave: the packet splits them into groups, the per-lane walk does not).  spp 3 in batches of 2 passes leaves a ragged
last batch.  Depth 1 is the camera launch alone (k_bounce in both orders), 2 adds the shade-only launch, 8 the rest.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

WALKS = (0, 1)
COUNTERS = ("segments", "nodes_tested", "prims_tested", "floor_tested")
SPP, PPB = 3, 2
N_BATCHES = (SPP + PPB - 1) // PPB


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


@pytest.fixture(scope="module")
def P():
    import path_tracer_ocaml_amd as P
    assert P.lib().ptx_device_count() >= 1, P.last_error()
    return P


def _desc(oracle, kind, w, h):
    return {"shirley": lambda: oracle.desc_shirley(w, h), "shirley_no_simd": lambda: oracle.desc_shirley(w, h, no_simd=True),
            "cornell": lambda: oracle.desc_cornell(w, h)}[kind]()


_REFS = {}


def _ref(oracle, kind, w, h, depth):
    """The oracle's render of a case, computed once and shared."""
    key = (kind, w, h, depth)
    if key not in _REFS:
        d = _desc(oracle, kind, w, h)
        _REFS[key] = (d, oracle.Scene(d.ptr, d).render(w, h, SPP, depth, threads=8, want_raw=True, count=True))
    return _REFS[key]


@pytest.mark.parametrize("depth", [1, 2, 8])
@pytest.mark.parametrize("w,h", [(13, 11), (72, 40)])
@pytest.mark.parametrize("kind", ["shirley", "shirley_no_simd", "cornell"])
def test_both_walks_against_the_oracle(P, oracle, kind, w, h, depth, monkeypatch):
    """Both walks x both bounce orders x {one wave takes every tile, the default workgroup} x one and two streams x counting and
    not counting (Simd_leaf: the C++ loop and the assembly loop)."""
    torch = pytest.importorskip("torch")
    monkeypatch.setenv("PTX_FUSED", "2")
    d, c = _ref(oracle, kind, w, h, depth)
    raw = torch.zeros((h, w, 3), dtype=torch.float64, device="cuda:0")
    got = {}
    for order in (0, 1):
        for threads, wgs in ((64, 1), (1024, 0)):
            for walk in WALKS:
                monkeypatch.setenv("PTX_BOUNCE_ORDER", str(order))
                monkeypatch.setenv("PTX_BOUNCE_THREADS", str(threads))
                monkeypatch.setenv("PTX_BOUNCE_WGS", str(wgs))
                monkeypatch.setenv("PTX_PRIMARY_WALK", str(walk))
                g = P.Scene(d.ptr, 0, keepalive=d)
                assert g.stats()["traversal_in_lds"] == 1
                for streams in ("1", "2"):
                    monkeypatch.setenv("PTX_STREAMS", streams)
                    for count in (True, False):
                        raw.zero_()
                        st = g.render_raw_device(P.render_params(w, h, SPP, depth, count_work=count, time_kernels=True, passes_per_batch=PPB),
                                                 raw.data_ptr())
                        r = raw.cpu().numpy()
                        where = (order, threads, walk, streams, count)
                        assert np.array_equal(bits(r), bits(c["raw"])), where
                        got[where[:2] + where[3:], walk] = r
                        if count:
                            for k in COUNTERS:
                                assert st[k] == c["counters"][k], (where, k, st[k], c["counters"][k])
                            assert st["primary_lane_walks"] == (N_BATCHES if walk == 1 else 0), (where, st["primary_lane_walks"])
                        kl = st["kernel_launches"]
                        assert kl["bounce"] == N_BATCHES * depth, (where, kl)
                        assert kl["trace"] == kl["shade"] == 0, (where, kl)
                g.close()
    for (combo, walk), r in got.items():
        if walk == 0:
            assert np.array_equal(bits(r), bits(got[combo, 1])), combo


@pytest.mark.parametrize("walk", WALKS)
def test_banded_shares_in_both_walks(P, oracle, walk, monkeypatch):
    """Three ranks' interleaved bands of 8 rows of a 40-row frame put together are the whole frame's raw sums."""
    torch = pytest.importorskip("torch")
    monkeypatch.setenv("PTX_PRIMARY_WALK", str(walk))
    w, h, depth = 72, 40, 8
    d, c = _ref(oracle, "shirley", w, h, depth)
    g = P.Scene(d.ptr, 0, keepalive=d)
    full = torch.zeros((h, w, 3), dtype=torch.float64, device="cuda:0")
    seen = np.zeros(h, dtype=int)
    lane_walks = 0
    for rank in range(3):
        pr = P.render_params(w, h, SPP, depth, band_rows=8, band_first=rank, band_step=3, passes_per_batch=PPB, count_work=True)
        rows = P.local_rows(pr)
        part = torch.zeros((rows, w, 3), dtype=torch.float64, device="cuda:0")
        st = g.render_raw_device(pr, part.data_ptr())
        lane_walks += st["primary_lane_walks"]
        for k in range(rows):
            gy = P.global_row(pr, k)
            full[gy] = part[k]
            seen[gy] += 1
    assert (seen == 1).all()
    assert np.array_equal(bits(full.cpu().numpy()), bits(c["raw"]))
    assert lane_walks == (3 * N_BATCHES if walk == 1 else 0)
    g.close()


@pytest.mark.parametrize("kind,per_lane", [("shirley", True), ("shirley_no_simd", False), ("cornell", False)])
def test_default_walk_by_scene(P, oracle, kind, per_lane, monkeypatch):
    """Without PTX_PRIMARY_WALK the Simd_leaf scene walks its camera rays one per lane and the Array_leaf scenes keep the packet."""
    torch = pytest.importorskip("torch")
    monkeypatch.delenv("PTX_PRIMARY_WALK", raising=False)
    w, h, depth = 72, 40, 8
    d, c = _ref(oracle, kind, w, h, depth)
    g = P.Scene(d.ptr, 0, keepalive=d)
    raw = torch.zeros((h, w, 3), dtype=torch.float64, device="cuda:0")
    st = g.render_raw_device(P.render_params(w, h, SPP, depth, count_work=True, passes_per_batch=PPB), raw.data_ptr())
    assert np.array_equal(bits(raw.cpu().numpy()), bits(c["raw"]))
    for k in COUNTERS:
        assert st[k] == c["counters"][k], k
    assert st["primary_lane_walks"] == (N_BATCHES if per_lane else 0)
    g.close()
