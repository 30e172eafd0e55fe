"""The two orders of a bounce launch on LDS-resident scenes (PTX_BOUNCE_ORDER, read when the scene handle is created):

  1            k_bounce_carry: launch b shades the hits its input entries carry (bounce b) and walks the new rays at once
               (bounce b + 1); survivors are binned by the category of the hit just found; the last launch only shades
  0            k_bounce: launch b walks bounce b, pools by category, shades bounce b
  2 (default)  by scene: 1 for scenes binned by elevation (Shirley), 0 for the others (cornell)

Only which wave does what when differs, and the order of a queue.  So the raw per-pixel sums are bit-identical between the
two and to the CPU oracle, every work counter is equal, and a batch is max_bounces launches in both.  ptx_stats.carry_launches
(counting renders) says which order ran.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ORDERS = (1, 0)
COUNTERS = ("segments", "nodes_tested", "prims_tested", "floor_tested")


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


# depth 1 (the walk-first kernel in both orders), 2 (camera launch + the shade-only launch), 3, 8, 16; workgroups of 64 .. 1024
# threads, the default grid and a handful of workgroups (hundreds of turns per wave: parking and resuming whole entries,
# part-filled blocks, holes); both fence scopes
CASES = [("shirley", 1, 0, 0, 0), ("shirley", 2, 64, 4, 1), ("shirley", 3, 1024, 2, 0), ("shirley", 8, 0, 0, 1), ("shirley", 8, 64, 4, 0),
         ("shirley", 16, 256, 16, 0), ("shirley", 16, 128, 1, 1), ("shirley", 2, 0, 0, 0),
         ("shirley_no_simd", 2, 128, 8, 0), ("shirley_no_simd", 3, 64, 2, 1), ("shirley_no_simd", 8, 0, 0, 1), ("shirley_no_simd", 16, 512, 3, 0),
         ("cornell", 1, 0, 0, 0), ("cornell", 2, 64, 2, 1), ("cornell", 3, 512, 3, 0), ("cornell", 8, 0, 0, 0), ("cornell", 8, 1024, 1, 1),
         ("cornell", 16, 64, 2, 1), ("cornell", 16, 256, 0, 0)]


@pytest.mark.parametrize("kind,depth,threads,wgs,fence_wg", CASES)
def test_both_orders_against_the_oracle(P, oracle, kind, depth, threads, wgs, fence_wg, monkeypatch):
    torch = pytest.importorskip("torch")
    monkeypatch.setenv("PTX_FUSED", "2")
    monkeypatch.setenv("PTX_BOUNCE_THREADS", str(threads))
    monkeypatch.setenv("PTX_BOUNCE_WGS", str(wgs))
    monkeypatch.setenv("PTX_BOUNCE_FENCE_WG", str(fence_wg))
    w, h, spp = 384, 192, 6
    d = _desc(oracle, kind, w, h)
    c = oracle.Scene(d.ptr, d).render(w, h, spp, depth, threads=8, want_raw=True, count=True)
    raw = torch.zeros((h, w, 3), dtype=torch.float64, device="cuda:0")
    got = {}
    for order in ORDERS:
        monkeypatch.setenv("PTX_BOUNCE_ORDER", str(order))
        g = P.Scene(d.ptr, 0, keepalive=d)
        assert g.stats()["traversal_in_lds"] == 1
        for streams in ("1", "2"):
            monkeypatch.setenv("PTX_STREAMS", streams)
            for count in (True, False):
                raw.zero_()
                st = g.render_raw_device(P.render_params(w, h, spp, depth, count_work=count, time_kernels=True, passes_per_batch=2), raw.data_ptr())
                r = raw.cpu().numpy()
                assert np.array_equal(bits(r), bits(c["raw"])), (order, streams, count)
                got[order] = r
                n_batches = (spp + 1) // 2
                if count:
                    for k in COUNTERS:
                        assert st[k] == c["counters"][k], (order, k)
                    # the order asked for is the one that ran (depth 1 has no second launch to carry a hit to)
                    assert st["carry_launches"] == (n_batches * depth if order == 1 and depth >= 2 else 0), (order, st["carry_launches"])
                kl = st["kernel_launches"]
                assert kl["bounce"] == n_batches * depth, (order, kl)
                assert kl["trace"] == kl["shade"] == 0, (order, kl)
        g.close()
    assert np.array_equal(bits(got[0]), bits(got[1]))


@pytest.mark.parametrize("order", ORDERS)
def test_queued_frames_in_both_orders(P, oracle, order, monkeypatch):
    """Frames of different depths queued back to back on one stream, nothing waited for in between: the workspace (both halves
    of the hit arrays) is reused in stream order."""
    torch = pytest.importorskip("torch")
    monkeypatch.setenv("PTX_BOUNCE_ORDER", str(order))
    w, h, spp = 320, 200, 6
    d = oracle.desc_shirley(w, h)
    g = P.Scene(d.ptr, 0, keepalive=d)
    stream = torch.cuda.current_stream().cuda_stream
    depths = (8, 3, 8, 2)
    got = [torch.full((h, w, 3), 7.0, dtype=torch.float64, device="cuda:0") for _ in depths]
    for depth, raw in zip(depths, got):
        g.render_raw_device(P.render_params(w, h, spp, depth, band_rows=8, asynchronous=True), raw.data_ptr(), stream)
    torch.cuda.synchronize()
    for depth, raw in zip(depths, got):
        c = oracle.Scene(d.ptr, d).render(w, h, spp, depth, threads=8, want_raw=True)
        assert np.array_equal(bits(raw.cpu().numpy()), bits(c["raw"])), depth
    g.close()


@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("kind", ["shirley", "cornell"])
def test_banded_shares_in_both_orders(P, oracle, kind, order, monkeypatch):
    """Three ranks' interleaved bands of 32 rows (ragged: 150 = 4 * 32 + 22) put together are the whole frame's raw sums."""
    torch = pytest.importorskip("torch")
    monkeypatch.setenv("PTX_BOUNCE_ORDER", str(order))
    w, h, spp, depth = 200, 150, 6, 8
    d = _desc(oracle, kind, w, h)
    c = oracle.Scene(d.ptr, d).render(w, h, spp, depth, threads=8, want_raw=True)
    g = P.Scene(d.ptr, 0, keepalive=d)
    full = torch.zeros((h, w, 3), dtype=torch.float64, device="cuda:0")
    seen = np.zeros(h, dtype=int)
    for rank in range(3):
        pr = P.render_params(w, h, spp, depth, band_rows=32, band_first=rank, band_step=3, passes_per_batch=4)
        rows = P.local_rows(pr)
        part = torch.zeros((rows, w, 3), dtype=torch.float64, device="cuda:0")
        g.render_raw_device(pr, part.data_ptr())
        for k in range(rows):
            gy = P.global_row(pr, k)
            full[gy] = part[k]
            seen[gy] += 1
    assert (seen == 1).all()
    assert np.array_equal(bits(full.cpu().numpy()), bits(c["raw"]))
    g.close()


@pytest.mark.parametrize("kind,carried", [("shirley", True), ("cornell", False)])
def test_default_order_by_scene(P, oracle, kind, carried, monkeypatch):
    """Without PTX_BOUNCE_ORDER the open scene takes the shade-first order and the closed box keeps the walk-first one."""
    torch = pytest.importorskip("torch")
    monkeypatch.delenv("PTX_BOUNCE_ORDER", raising=False)
    w, h, spp, depth = 256, 128, 4, 5
    d = _desc(oracle, kind, w, h)
    c = oracle.Scene(d.ptr, d).render(w, h, spp, depth, threads=8, want_raw=True, count=True)
    g = P.Scene(d.ptr, 0, keepalive=d)
    raw = torch.zeros((h, w, 3), dtype=torch.float64, device="cuda:0")
    st = g.render_raw_device(P.render_params(w, h, spp, depth, count_work=True, time_kernels=True, passes_per_batch=2), raw.data_ptr())
    assert np.array_equal(bits(raw.cpu().numpy()), bits(c["raw"]))
    assert st["kernel_launches"]["bounce"] == 2 * depth
    assert st["carry_launches"] == (2 * depth if carried else 0)
    g.close()
