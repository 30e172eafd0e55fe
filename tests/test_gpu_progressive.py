"""Progressive rendering on the GPU, bit for bit where the data allows it.

The sampler offset of a sample depends only on (x, y, pass, N) (integrator.ml:98) and the raw sums add the passes in order, so
* any partition of [0, N) into slices (ptx_render_passes_device) gives the one-shot frame's raw sums, bit for bit;
* after k passes the sums are the pass-order prefix sums of the oracle's per-sample radiance, and the square sums the prefix
  sums of c * c; the per-pixel error and rel_err follow from them by the documented formula;
* update k of ptx_render_progressive is ptx_film_resolve_device(raw_k, spp = k), and the last one is ptx_render's frame.
Scenes: Shirley (Simd_leaf, tree in LDS), cornell with its emitter, a ganesha-like mesh walked from HBM.
"""
import os
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H, N = 64, 48, 16
DEPTH = {"shirley": 8, "cornell": 16, "ganesha": 8}


def bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


@pytest.fixture(scope="module")
def P():
    import path_tracer_ocaml_amd as P
    assert P.lib().ptx_device_count() >= 1, P.last_error()
    return P


@pytest.fixture(scope="module")
def torch():
    return pytest.importorskip("torch")


@pytest.fixture(scope="module")
def scenes(P, oracle):
    made = {"shirley": oracle.desc_shirley(W, H), "cornell": oracle.desc_cornell(W, H),
            "ganesha": oracle.desc_ganesha_like(W, H, n_target=40000)}
    out = {k: (d, P.Scene(d.ptr, 0, keepalive=d)) for k, d in made.items()}
    assert out["shirley"][1].stats()["traversal_in_lds"]
    assert not out["ganesha"][1].stats()["traversal_in_lds"]
    yield out
    for _, g in out.values():
        g.close()


def _zeros(torch, rows, w=W):
    return torch.zeros((rows, w, 3), dtype=torch.float64, device="cuda:0")


def _partitions(rng, n, count):
    """`count` random partitions of [0, n) into consecutive slices (one of them single passes)"""
    out = [[(k, k + 1) for k in range(n)]]
    for _ in range(count):
        cuts = sorted(rng.choice(np.arange(1, n), size=int(rng.integers(1, n - 1)), replace=False).tolist())
        edges = [0] + cuts + [n]
        out.append(list(zip(edges[:-1], edges[1:])))
    return out


@pytest.mark.parametrize("kind", ["shirley", "cornell", "ganesha"])
def test_slices_equal_the_one_shot_frame(P, torch, scenes, kind):
    _, g = scenes[kind]
    rng = np.random.default_rng(11)
    depth = DEPTH[kind]
    # passes_per_batch 2: a slice of 3+ passes is two batches or more on two streams; 5 and 0 give batches that the slices cut
    for ppb in (0, 2, 5):
        params = P.render_params(W, H, N, depth, passes_per_batch=ppb)
        whole = _zeros(torch, H)
        g.render_raw_device(params, whole.data_ptr())
        for i, part in enumerate(_partitions(rng, N, 3)):
            raw, sq = _zeros(torch, H), _zeros(torch, H)
            for a, b in part:
                st = g.render_passes_device(params, a, b - a, raw.data_ptr(), sq.data_ptr() if i % 2 == 0 else None)
                assert st["samples"] == W * H * (b - a)
            assert torch.equal(raw.view(torch.int64), whole.view(torch.int64)), (kind, ppb, part)
            if i % 2 == 0:
                assert float(sq.max()) > 0.0
    assert float(whole.max()) > 0.0
    # three band-sharded ranks: each rank's slices add up to its share of the one-shot frame
    for rank in range(3):
        params = P.render_params(W, H, N, depth, band_rows=8, band_first=rank, band_step=3, passes_per_batch=3)
        rows = P.local_rows(params)
        whole, raw = _zeros(torch, rows), _zeros(torch, rows)
        g.render_raw_device(params, whole.data_ptr())
        for a, b in ((0, 7), (7, 8), (8, 16)):
            g.render_passes_device(params, a, b - a, raw.data_ptr())
        assert torch.equal(raw.view(torch.int64), whole.view(torch.int64)), (kind, rank)


def test_slices_are_queued_on_the_callers_stream_with_async(P, torch, scenes):
    """PTX_RENDER_ASYNC: slices queued back to back on a torch stream, then one wait -- the same sums"""
    _, g = scenes["shirley"]
    whole = _zeros(torch, H)
    g.render_raw_device(P.render_params(W, H, N, 8), whole.data_ptr())
    params = P.render_params(W, H, N, 8, asynchronous=True, passes_per_batch=2)
    s = torch.cuda.Stream()
    raw, sq = _zeros(torch, H), _zeros(torch, H)
    torch.cuda.synchronize()
    for a, b in ((0, 5), (5, 6), (6, 16)):
        g.render_passes_device(params, a, b - a, raw.data_ptr(), sq.data_ptr(), stream=s.cuda_stream)
    s.synchronize()
    assert torch.equal(raw.view(torch.int64), whole.view(torch.int64))


def test_pass_ranges_are_checked(P, torch, scenes):
    _, g = scenes["shirley"]
    params = P.render_params(W, H, N, 8)
    raw = _zeros(torch, H)
    for a, n in ((-1, 2), (0, 0), (15, 2), (16, 1), (0, N + 1), (3, -1)):
        with pytest.raises(P.PtxError, match="pass"):
            g.render_passes_device(params, a, n, raw.data_ptr())
    assert float(raw.abs().max()) == 0.0
    with pytest.raises(P.PtxError, match="passes_done"):
        P.pixel_error_device(0, W, H, 0, raw.data_ptr(), raw.data_ptr())


def _oracle_prefix(oracle, d, n, depth, k):
    """numpy pass-order prefix sums (S1, S2) of the oracle's per-sample radiance over passes [0, k) of an n-pass frame"""
    ys, xs, ps = np.meshgrid(np.arange(H), np.arange(W), np.arange(k), indexing="ij")
    rgb, _ = oracle.Scene(d.ptr, d).trace_samples(W, H, n, depth, xs.ravel(), ys.ravel(), ps.ravel())
    per = rgb.reshape(H, W, k, 3)
    s1, s2 = np.zeros((H, W, 3)), np.zeros((H, W, 3))
    for p in range(k):
        c = per[:, :, p]
        s1 = s1 + c
        s2 = s2 + c * c
    return s1, s2


def _se(s1, s2, k):
    return np.sqrt(np.maximum(0.0, s2 - s1 * s1 / k) / (k * (k - 1)))


@pytest.mark.parametrize("kind", ["shirley", "cornell", "ganesha"])
def test_prefix_equals_the_oracle(P, torch, oracle, scenes, kind):
    d, g = scenes[kind]
    depth = DEPTH[kind]
    params = P.render_params(W, H, N, depth, passes_per_batch=3)
    raw, sq, err = _zeros(torch, H), _zeros(torch, H), _zeros(torch, H)
    done = 0
    for k in (1, 2, 7, N):
        g.render_passes_device(params, done, k - done, raw.data_ptr(), sq.data_ptr())
        done = k
        s1, s2 = _oracle_prefix(oracle, d, N, depth, k)
        assert np.array_equal(bits(raw.cpu().numpy()), bits(s1)), (kind, k)
        assert np.array_equal(bits(sq.cpu().numpy()), bits(s2)), (kind, k)
        rel = P.pixel_error_device(0, W, H, k, raw.data_ptr(), sq.data_ptr(), err.data_ptr())
        got = err.cpu().numpy()
        if k < 2:
            assert np.isinf(got).all() and got.min() > 0 and rel == float("inf")
            continue
        want = _se(s1, s2, k)
        np.testing.assert_allclose(got, want, rtol=1e-12, atol=0)
        want_rel = np.sqrt((want * want).sum()) / np.sqrt(((s1 / k) ** 2).sum())
        assert abs(rel - want_rel) <= 1e-12 * want_rel, (rel, want_rel)
        assert 0.0 < rel < 10.0
        # the same sums give the same bits (fixed-order reduction, no atomics)
        rel2 = P.pixel_error_device(0, W, H, k, raw.data_ptr(), sq.data_ptr())
        assert np.float64(rel).view(np.uint64) == np.float64(rel2).view(np.uint64)
    assert float(s1.max()) > 0.0


def test_prefix_is_not_the_smaller_frame(P, torch, scenes):
    """8 passes of a 32-pass frame are NOT the 8-pass frame: N fixes the sampler offsets (y*W + x + pass*N)"""
    _, g = scenes["shirley"]
    prefix, small = _zeros(torch, H), _zeros(torch, H)
    g.render_passes_device(P.render_params(W, H, 32, 8), 0, 8, prefix.data_ptr())
    g.render_raw_device(P.render_params(W, H, 8, 8), small.data_ptr())
    assert not torch.equal(prefix.view(torch.int64), small.view(torch.int64))


def test_pixel_error_of_zero_sums_is_zero(P, torch):
    z = _zeros(torch, 5, 7)
    err = _zeros(torch, 5, 7) - 1.0
    assert P.pixel_error_device(0, 7, 5, 4, z.data_ptr(), z.data_ptr(), err.data_ptr()) == 0.0
    assert float(err.abs().max()) == 0.0


@pytest.mark.parametrize("kind", ["shirley", "cornell", "ganesha"])
def test_updates_film_the_running_sums(P, torch, oracle, scenes, kind):
    d, g = scenes[kind]
    depth = DEPTH[kind]
    seen = []
    rgb, err, done, st = g.render_progressive(W, H, N, depth, 5, on_update=lambda k, rel, im, e: seen.append(
        (k, rel, im.copy(), e.copy())))
    assert [s[0] for s in seen] == [5, 10, 15, 16] and done == 16
    assert st["samples"] == W * H * N
    params = P.render_params(W, H, N, depth)
    for k, rel, im, e in seen:
        raw, sq, rgb_d, err_d = _zeros(torch, H), _zeros(torch, H), _zeros(torch, H), _zeros(torch, H)
        g.render_passes_device(params, 0, k, raw.data_ptr(), sq.data_ptr())
        P.film_resolve_device(0, W, H, k, raw.data_ptr(), rgb_d.data_ptr())
        assert np.array_equal(bits(im), bits(rgb_d.cpu().numpy())), (kind, k)
        want_rel = P.pixel_error_device(0, W, H, k, raw.data_ptr(), sq.data_ptr(), err_d.data_ptr())
        assert np.float64(rel).view(np.uint64) == np.float64(want_rel).view(np.uint64)
        assert np.array_equal(bits(e), bits(err_d.cpu().numpy()))
    assert np.array_equal(bits(rgb), bits(seen[-1][2])) and np.array_equal(bits(err), bits(seen[-1][3]))
    ref, _ = g.render(W, H, N, depth)
    assert np.array_equal(bits(rgb), bits(ref)), kind
    orc = oracle.Scene(d.ptr, d).render(W, H, N, depth, threads=8)["rgb"]
    assert float((np.abs(rgb - orc) / np.maximum(np.abs(orc), 1e-3)).max()) <= 1e-12
    # without the error: the same images, rel_err NaN, no err
    seen2 = []
    rgb2, err2, done2, _ = g.render_progressive(W, H, N, depth, 5, want_error=False,
                                                on_update=lambda k, rel, im, e: seen2.append((k, rel, e)))
    assert err2 is None and done2 == N and np.array_equal(bits(rgb2), bits(ref))
    assert [s[0] for s in seen2] == [5, 10, 15, 16] and all(np.isnan(s[1]) and s[2] is None for s in seen2)


def test_pinned_image_and_the_integrator(P, scenes):
    from path_tracer_ocaml_amd import integrator as I
    _, g = scenes["shirley"]
    ref, _ = g.render(W, H, N, 8)
    img = np.full((H, W, 3), -1.0)
    g.pin_image(img)
    try:
        seen = []
        out, _, done, _ = g.render_progressive(W, H, N, 8, 6, out=img, on_update=lambda k, rel, im, e: seen.append(im is img))
    finally:
        g.unpin_image()
    assert out is img and done == N and seen == [True, True, True]
    assert np.array_equal(bits(img), bits(ref))
    image = np.zeros((H, W, 3))
    integ = I.Integrator.create(width=W, height=H, image=image, samples_per_pixel=N, max_bounces=8, scene=g)
    assert integ.render_progressive(4) is image
    assert integ.passes_done == N and integ.error.shape == (H, W, 3)
    assert np.array_equal(bits(image), bits(ref))


def test_callback_stops_the_render(P, oracle, scenes):
    d, g = scenes["cornell"]
    depth = DEPTH["cornell"]
    seen = []

    def stop_at_second(k, rel, im, e):
        seen.append((k, im.copy()))
        return len(seen) == 2

    rgb, err, done, st = g.render_progressive(W, H, N, depth, 4, on_update=stop_at_second)
    assert done == 8 and [s[0] for s in seen] == [4, 8]
    assert st["samples"] == W * H * 8
    assert np.array_equal(bits(rgb), bits(seen[1][1]))
    # the handle renders whole frames as before
    after, _ = g.render(W, H, N, depth)
    fresh = P.Scene(d.ptr, 0, keepalive=d)
    try:
        want, _ = fresh.render(W, H, N, depth)
    finally:
        fresh.close()
    assert np.array_equal(bits(after), bits(want))


def test_target_error_stops_at_the_same_update_every_time(P, scenes):
    _, g = scenes["cornell"]
    depth = DEPTH["cornell"]
    rels = []
    g.render_progressive(W, H, N, depth, 2, on_update=lambda k, rel, im, e: rels.append((k, rel)))
    assert [k for k, _ in rels] == list(range(2, N + 1, 2))
    assert rels[0][1] > rels[-1][1] > 0.0
    target = rels[3][1]  # the first update at or below it is the 4th (rel_err falls with k)
    first = next(k for k, r in rels if r <= target)
    runs = [g.render_progressive(W, H, N, depth, 2, target_rel_err=target) for _ in range(2)]
    for rgb, err, done, st in runs:
        assert done == first and st["samples"] == W * H * first
    assert np.array_equal(bits(runs[0][0]), bits(runs[1][0])) and np.array_equal(bits(runs[0][1]), bits(runs[1][1]))


def test_python_callback_exception_is_raised_again(P, scenes):
    _, g = scenes["shirley"]
    calls = []

    class Boom(Exception):
        pass

    def cb(k, rel, im, e):
        calls.append(k)
        raise Boom(k)

    with pytest.raises(Boom):
        g.render_progressive(W, H, N, 8, 4, on_update=cb)
    assert calls == [4]
    ref, _ = g.render(W, H, N, 8)  # the handle is usable afterwards
    assert float(ref.max()) > 0.5


def test_cli_progressive_writes_the_plain_runs_png(tmp_path):
    exe = os.path.join(ROOT, "path_tracer_ocaml_amd", "shirley_spheres")
    env = dict(os.environ)
    env["LD_LIBRARY_PATH"] = "/opt/rocm/lib:" + env.get("LD_LIBRARY_PATH", "")
    base = [exe, "--dimension=600,300", "--samples-per-pixel=32", "--max-ray-bounces=8", "--no-progress"]
    plain, prog = tmp_path / "plain.png", tmp_path / "prog.png"
    r0 = subprocess.run(base + ["-o", str(plain)], capture_output=True, text=True, env=env, timeout=300)
    assert r0.returncode == 0, r0.stderr
    r1 = subprocess.run(base + ["--progressive=4", "-o", str(prog)], capture_output=True, text=True, env=env, timeout=300)
    assert r1.returncode == 0, r1.stderr
    assert prog.read_bytes() == plain.read_bytes()
    updates = [l for l in r1.stdout.splitlines() if l.startswith("#passes = ")]
    assert [int(l.split(",")[0].split("=")[1]) for l in updates] == list(range(4, 33, 4))
    errs = [float(l.split("error = ")[1]) for l in updates]
    assert all(0.0 < e < float("inf") for e in errs) and errs[-1] < errs[0]
    assert "#passes" not in r0.stdout
    assert any(l.startswith("rendered in: ") for l in r1.stdout.splitlines())
    # the plain run's lines are all there, in order, around the updates (timings aside)
    def fixed(out):
        return [l for l in out.splitlines() if not l.startswith(("#passes", "build time", "rendered in", "throughput"))]
    assert fixed(r1.stdout) == fixed(r0.stdout) and len(fixed(r0.stdout)) >= 4
    # --target-error stops at the first update that meets it (the printed errors have 6 digits: a target just above the third)
    target = errs[2] * (1 + 1e-5)
    assert errs[0] > target and errs[1] > target
    r2 = subprocess.run(base + ["--progressive=4", f"--target-error={target!r}", "-o", str(tmp_path / "t.png")],
                        capture_output=True, text=True, env=env, timeout=300)
    assert r2.returncode == 0, r2.stderr
    assert [l for l in r2.stdout.splitlines() if l.startswith("#passes = ")] == updates[:3]
