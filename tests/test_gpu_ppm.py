"""Progressive photon mapping on the GPU against the oracle's restatement of
progressive-photon-map/src/progressive_photon_map.ml.  No fixture of the reference pins this integrator
(parity unpinned); the bar here is GPU == oracle: photon counts and ray counts exact, neighbour counts exact,
img_sum bit-exact (the photon list order, the photon tree and the summation order are all reproduced).
The oracle itself is held to a brute-force gather, exact radii and the lights' rays in test_ppm_oracle.py; the cases below
sit on the sizes at which this code changes path (scan tile, device list / tree, root segment class), on the per-thread
builder workspace, on the iteration callback and on the edges of the argument space, and one compares the GPU's image with
the brute-force reference directly."""
import numpy as np
import pytest

import ppm_reference as R

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def P():
    import path_tracer_ocaml_amd as P
    assert P.lib().ptx_device_count() >= 1, P.last_error()
    return P


def _check(P, oracle, desc, lights, params):
    o = oracle.Scene(desc.ptr, desc)
    g = P.Scene(desc.ptr, 0, keepalive=desc)
    o_img, o_st = o.ppm_render(params, lights)
    g_img, g_st = g.ppm_render(params, lights)
    for k in ("photons_stored", "photon_rays", "eye_rays", "neighbors"):
        assert g_st[k] == o_st[k], (k, g_st[k], o_st[k])
    assert g_st["last_radius"] == o_st["last_radius"]
    assert o_img.max() > 0
    nbad = int((g_img.view(np.uint64) != o_img.view(np.uint64)).sum())
    assert nbad == 0, f"{nbad} of {o_img.size} img_sum values differ from the oracle"
    g.close()
    return o_img, o_st


def _builders(P, desc, lights, params):
    """(device_trees, gpu_built_trees) of a run: which builder made the photon trees (a failed GPU build falls back to the host's
    builder with the same tree, so the image cannot tell)."""
    g = P.Scene(desc.ptr, 0, keepalive=desc)
    _, st = g.ppm_render(params, lights)
    g.close()
    return st["device_trees"], st["gpu_built_trees"]


def test_ppm_cornell_point_light(P, oracle):
    from path_tracer_ocaml_amd import abi
    w = h = 160
    d = oracle.desc_cornell(w, h, 0.0)  # the reference's scene: no emitter, a point light
    img, st = _check(P, oracle, d, oracle.lights_cornell(w, h), abi.ppm_params(w, h, iterations=3, photon_count=20000))
    assert st["photons_stored"] > 50000 and st["neighbors"] > 1_000_000


def test_ppm_host_side_list_and_tree(P, oracle, monkeypatch):
    """PTX_PPM_HOST_LIST=1: the photon list and the photon tree are made on the host (the path small maps take)."""
    from path_tracer_ocaml_amd import abi
    monkeypatch.setenv("PTX_PPM_HOST_LIST", "1")
    w = h = 96
    d = oracle.desc_cornell(w, h, 0.0)
    _check(P, oracle, d, oracle.lights_cornell(w, h), abi.ppm_params(w, h, iterations=2, photon_count=12000))


def test_ppm_small_map_below_gpu_build_threshold(P, oracle):
    from path_tracer_ocaml_amd import abi
    w = h = 64
    d = oracle.desc_cornell(w, h, 0.0)
    _, st = _check(P, oracle, d, oracle.lights_cornell(w, h), abi.ppm_params(w, h, iterations=2, photon_count=2000))
    assert st["photons_stored"] < 2 * 8192


def test_ppm_ganesha_like_two_spot_lights(P, oracle):
    from path_tracer_ocaml_amd import abi
    w, h = 160, 90
    d = oracle.desc_ganesha_like(w, h, 20000)
    d.d.background.kind = abi.PTX_BG_BLACK
    lights = oracle.Scene(d.ptr, d).lights_ganesha()
    _check(P, oracle, d, lights, abi.ppm_params(w, h, iterations=2, photon_count=30000, max_bounces=4))


def test_ppm_shirley_simd_leaf_one_bounce_deep(P, oracle):
    """The photon pass on the Simd_leaf scene, deeper paths, alpha at its default."""
    from path_tracer_ocaml_amd import abi
    w, h = 120, 60
    d = oracle.desc_shirley(w, h)
    light = abi.Light()
    light.kind = abi.PTX_LIGHT_POINT
    light.position[:] = [0.0, 6.0, -12.0]
    light.color[:] = [1.0, 0.9, 0.8]
    light.power = 50.0
    _check(P, oracle, d, [light], abi.ppm_params(w, h, iterations=2, photon_count=15000, max_bounces=8))


# ---- image textures and the environment in the photon mapper (the IMG instantiations of both passes) ----
def _ppm_image_check(P, oracle, src, index, cells, lights, params):
    """the even checker on entry `index` as an image (nearest, repeat on both axes) on the GPU against the oracle on the checker
    descriptor: img_sum bit for bit, the stats equal.  Returns (the GPU scene with the image set, the oracle's image)."""
    import ctypes as C
    import texture_reference as T
    import texture_support as S
    d, keep = S.with_checker(src, index, cells[0] + 1, cells[1] + 1)
    o = oracle.Scene(C.pointer(d), keep)
    o_img, o_st = o.ppm_render(params, lights)
    o.close()
    even, odd = S.checker_colours(d, index)
    g = P.Scene(C.pointer(d), 0, keepalive=keep)
    g.set_texture_image(index, T.checker_image(cells[0], cells[1], even, odd), repeat=(True, True))
    g_img, g_st = g.ppm_render(params, lights)
    for k in ("photons_stored", "photon_rays", "eye_rays", "neighbors", "last_radius"):
        assert g_st[k] == o_st[k], (k, g_st[k], o_st[k])
    assert o_img.max() > 0
    nbad = int((g_img.view(np.uint64) != o_img.view(np.uint64)).sum())
    assert nbad == 0, f"{nbad} of {o_img.size} img_sum values differ from the oracle"
    return g, o_img


@pytest.mark.parametrize("host_list", [False, True])
def test_ppm_cornell_with_a_checker_image(P, oracle, monkeypatch, host_list):
    """Array_leaf mode, the shape of test_ppm_host_side_list_and_tree, on both list paths; then the controls: an image that is not
    the checker (its two colours exchanged) gives another img_sum, removing it the checker's bits again"""
    import texture_reference as T
    import texture_support as S
    from path_tracer_ocaml_amd import abi
    if host_list:
        monkeypatch.setenv("PTX_PPM_HOST_LIST", "1")
    w = h = 96
    lights, params = oracle.lights_cornell(w, h), abi.ppm_params(w, h, iterations=2, photon_count=12000)
    g, o_img = _ppm_image_check(P, oracle, oracle.desc_cornell(w, h, 0.0), 4, (10, 10), lights, params)
    try:
        if not host_list:
            even, odd = S.checker_colours(oracle.desc_cornell(w, h, 0.0).d, 4)  # (with_checker keeps a checker entry's colours)
            g.set_texture_image(4, T.checker_image(10, 10, odd, even), repeat=(True, True))
            other, _ = g.ppm_render(params, lights)
            assert not np.array_equal(other, o_img)
            g.set_texture_image(4, None)
            back, _ = g.ppm_render(params, lights)
            assert np.array_equal(back.view(np.uint64), o_img.view(np.uint64))
    finally:
        g.close()


def test_ppm_shirley_simd_leaf_with_a_checker_image(P, oracle):
    """the PT_MODE_SIMD instantiations: the checker on the ground, the lights and shape of
    test_ppm_shirley_simd_leaf_one_bounce_deep"""
    from path_tracer_ocaml_amd import abi
    w, h = 120, 60
    light = abi.Light()
    light.kind = abi.PTX_LIGHT_POINT
    light.position[:] = [0.0, 6.0, -12.0]
    light.color[:] = [1.0, 0.9, 0.8]
    light.power = 50.0
    g, _ = _ppm_image_check(P, oracle, oracle.desc_shirley(w, h), 0, (10, 20), [light],
                            abi.ppm_params(w, h, iterations=2, photon_count=15000, max_bounces=8))
    g.close()


def test_ppm_ignores_an_environment(P, oracle):
    """a miss ends a photon path and an eye path, so an environment alone changes nothing: the oracle's bits"""
    import texture_support as S
    from path_tracer_ocaml_amd import abi
    w = h = 48
    d = oracle.desc_cornell(w, h, 0.0)
    lights, params = oracle.lights_cornell(w, h), abi.ppm_params(w, h, iterations=2, photon_count=4000)
    o_img, o_st = oracle.Scene(d.ptr, d).ppm_render(params, lights)
    g = P.Scene(d.ptr, 0, keepalive=d)
    g.set_environment(S.random_environment(16, 8, 5), rotation=S.rotation([0.3, 1.0, 0.2], 50.0))
    g_img, g_st = g.ppm_render(params, lights)
    g.close()
    assert o_img.max() > 0 and np.array_equal(g_img.view(np.uint64), o_img.view(np.uint64))
    for k in ("photons_stored", "photon_rays", "eye_rays", "neighbors", "last_radius"):
        assert g_st[k] == o_st[k], k


def test_ppm_rejects_bad_arguments(P, oracle):
    from path_tracer_ocaml_amd import abi
    d = oracle.desc_cornell(16, 16, 0.0)
    g = P.Scene(d.ptr, 0, keepalive=d)
    with pytest.raises(P.PtxError):
        g.ppm_render(abi.ppm_params(16, 16, iterations=0), oracle.lights_cornell(16, 16))
    bad = abi.Light()
    bad.kind = 7
    with pytest.raises(P.PtxError):
        g.ppm_render(abi.ppm_params(16, 16, iterations=1, photon_count=100), [bad])
    # the light table: every one of these is turned away on the host with PTX_ERR_ARG (-1), before anything is allocated or
    # launched
    good = oracle.lights_cornell(16, 16)[0]
    p = abi.ppm_params(16, 16, iterations=1, photon_count=100)
    nan, inf = float("nan"), float("inf")

    def light(kind=abi.PTX_LIGHT_POINT, power=2.0, color=(1.0, 1.0, 1.0), position=None, direction=(0.0, 0.0, 1.0)):
        l = abi.Light()
        l.kind, l.power = kind, power
        l.color[:] = list(color)
        l.position[:] = list(position) if position is not None else list(good.position)
        l.direction[:] = list(direction)
        return l

    tables = {
        "nan power": [light(power=nan)], "inf power": [light(power=inf)], "-inf power": [light(power=-inf)],
        "nan colour": [light(color=(1.0, nan, 1.0))], "inf colour": [light(color=(inf, 1.0, 1.0))],
        "nan position": [light(position=(0.0, nan, 0.0))], "inf position": [light(position=(0.0, 0.0, -inf))],
        "negative power": [light(power=-1.0)], "negative colour": [light(color=(1.0, -0.5, 1.0))],
        "negative second light": [good, light(power=-0.25)], "nan second light": [good, light(power=nan)],
        "power x colour overflows": [light(power=1e200, color=(1e200, 1.0, 1.0))],
        "zero total": [light(power=0.0), light(color=(0.0, 0.0, 0.0))],
        "zero spot direction": [light(kind=abi.PTX_LIGHT_SPOT, direction=(0.0, 0.0, 0.0))],
        "nan spot direction": [light(kind=abi.PTX_LIGHT_SPOT, direction=(0.0, nan, 1.0))],
    }
    for what, table in tables.items():
        with pytest.raises(P.PtxError, match=r"\(-1\)"):
            g.ppm_render(p, table)
            pytest.fail(f"{what}: accepted")
    # and the scene is none the worse for it
    o_img, o_st = oracle.Scene(d.ptr, d).ppm_render(p, [good])
    g_img, g_st = g.ppm_render(p, [good])
    assert np.array_equal(g_img.view(np.uint64), o_img.view(np.uint64)) and g_st["neighbors"] == o_st["neighbors"]
    g.close()


# ---- sizes at which the code changes path ----
@pytest.mark.parametrize("photon_count", [1, 255, 1023, 1024, 1025, 2049, 4097, 5119, 5120, 5121])
def test_ppm_scan_tiles(P, oracle, photon_count):
    """The three-pass scan of the deposit counts works in tiles of 1024 paths.  What the scan writes (the list order and the photon
    boxes) is gathered from only when the list holds >= 4096 photons; below that the host rebuilds the list and reads no more
    than the scan's total.  So the scan itself is pinned by 4097 (four tiles and a path) and by 5119 / 5120 / 5121 (one short of
    five tiles, exactly five, five and a path), which store 7365 and about 9178 photons and must report a device-resident tree.
    The small counts (one path, one short of a wave's four, either side of one tile, two tiles and a path) exercise the tails of
    the photon kernel's grid and the scan's total on the host-list path."""
    from path_tracer_ocaml_amd import abi
    w = h = 24
    d = oracle.desc_cornell(w, h, 0.0)
    p = abi.ppm_params(w, h, iterations=1, photon_count=photon_count, max_bounces=4)
    _, st = _check(P, oracle, d, oracle.lights_cornell(w, h), p)
    if photon_count >= 4097:
        assert st["photons_stored"] >= 4096
    assert _builders(P, d, oracle.lights_cornell(w, h), p) == ((1, 1) if st["photons_stored"] >= 4096 else (0, 0))


_THRESHOLDS = {}


def _photon_count_storing(oracle, target):
    """The photon_count at which iteration 0 of the 8x8 cornell scene stores exactly `target` photons with max_bounces = 1: a path
    then stores 0 or 1 photon and the paths do not depend on photon_count, so the stored count is monotone in steps of at most
    1 and bisection on the oracle finds every target."""
    from path_tracer_ocaml_amd import abi
    if not _THRESHOLDS:
        w = h = 8
        d = oracle.desc_cornell(w, h, 0.0)
        sc, lights = oracle.Scene(d.ptr, d), oracle.lights_cornell(w, h)
        seen = {}

        def stored(pc):
            if pc not in seen:
                seen[pc] = sc.ppm_render(abi.ppm_params(w, h, iterations=1, photon_count=pc, max_bounces=1), lights)[1]["photons_stored"]
            return seen[pc]

        for t in (4095, 4096, 4097, 8191, 8192):
            lo, hi = 1, 1 << 16
            assert stored(hi) >= t
            while lo < hi:
                mid = (lo + hi) // 2
                if stored(mid) >= t:
                    hi = mid
                else:
                    lo = mid + 1
            assert stored(lo) == t
            _THRESHOLDS[t] = lo
        print("photon_count per stored-photon threshold:", _THRESHOLDS)
    return _THRESHOLDS[target]


@pytest.mark.parametrize("host_list", [False, True])
@pytest.mark.parametrize("stored", [4095, 4096, 4097, 8191, 8192])
def test_ppm_stored_photon_thresholds(P, oracle, monkeypatch, stored, host_list):
    """4096 stored photons: the device list / tree and the GPU builder take over from the host's; 8192: the builder's root segment
    changes class.  Each side of both, with the list made on the device and (PTX_PPM_HOST_LIST=1) on the host."""
    from path_tracer_ocaml_amd import abi
    pc = _photon_count_storing(oracle, stored)
    if host_list:
        monkeypatch.setenv("PTX_PPM_HOST_LIST", "1")
    w = h = 8
    d = oracle.desc_cornell(w, h, 0.0)
    p = abi.ppm_params(w, h, iterations=1, photon_count=pc, max_bounces=1)
    _, st = _check(P, oracle, d, oracle.lights_cornell(w, h), p)
    assert st["photons_stored"] == stored
    # which builder ran: from 4096 photons on the GPU builder makes the tree, and without the host list it never leaves the device
    want = (0, 0) if stored < 4096 else (0, 1) if host_list else (1, 1)
    assert _builders(P, d, oracle.lights_cornell(w, h), p) == want


def test_ppm_builder_workspace_reuse_on_one_thread(P, oracle):
    """The photon tree is rebuilt every iteration into the calling thread's builder workspace, which scene creation with the GPU
    builder uses too: a small map after a large one, a scene built in between and a second scene interleaved must all leave
    nothing behind."""
    import ctypes as C
    from path_tracer_ocaml_amd import abi
    w = h = 32
    d1, d2 = oracle.desc_cornell(w, h, 0.0), oracle.desc_cornell(40, 24, 0.0)
    l1, l2 = oracle.lights_cornell(w, h), oracle.lights_cornell(40, 24)
    o1, o2 = oracle.Scene(d1.ptr, d1), oracle.Scene(d2.ptr, d2)
    g1, g2 = P.Scene(d1.ptr, 0, keepalive=d1), P.Scene(d2.ptr, 0, keepalive=d2)

    def both(o, g, params, lights):
        o_img, o_st = o.ppm_render(params, lights)
        g_img, g_st = g.ppm_render(params, lights)
        for k in ("photons_stored", "photon_rays", "eye_rays", "neighbors", "last_radius"):
            assert g_st[k] == o_st[k], (k, g_st[k], o_st[k])
        assert np.array_equal(g_img.view(np.uint64), o_img.view(np.uint64))
        return g_img

    small = abi.ppm_params(w, h, iterations=2, photon_count=5000)
    first = both(o1, g1, small, l1)
    both(o2, g2, abi.ppm_params(40, 24, iterations=1, photon_count=7000), l2)
    both(o1, g1, abi.ppm_params(w, h, iterations=2, photon_count=20000), l1)
    od = oracle.desc_ganesha_like(64, 36, 9000)
    dd = abi.SceneDesc()
    C.memmove(C.byref(dd), od.ptr, C.sizeof(dd))
    ob, oi, oo = oracle.Scene(C.pointer(dd), od).tree()
    dd.reserved = 2  # GPU builder
    gg = P.Scene(dd, 0, keepalive=od)
    gb, gi, go = gg.tree()
    assert np.array_equal(gb.view(np.uint64), ob.view(np.uint64)) and np.array_equal(gi, oi) and np.array_equal(go, oo)
    both(o2, g2, abi.ppm_params(40, 24, iterations=1, photon_count=3000), l2)
    third = both(o1, g1, small, l1)
    assert np.array_equal(first.view(np.uint64), third.view(np.uint64))
    for g in (g1, g2, gg):
        g.close()


def test_ppm_iteration_callback(P, oracle):
    """Scene.ppm_render(callback=): callback k sees iteration k's radius and list length (the oracle's) and an image that is the
    k + 1 iteration run's, bit for bit."""
    from path_tracer_ocaml_amd import abi
    w = h = 24
    d = oracle.desc_cornell(w, h, 0.0)
    lights = oracle.lights_cornell(w, h)
    o, g = oracle.Scene(d.ptr, d), P.Scene(d.ptr, 0, keepalive=d)
    params = lambda n: abi.ppm_params(w, h, iterations=n, photon_count=3000)  # noqa: E731
    seen = []
    img, st = g.ppm_render(params(4), lights, callback=lambda *a: seen.append(a))
    assert [a[0] for a in seen] == [0, 1, 2, 3]
    for k, (_, radius, length, image) in enumerate(seen):
        dmp = o.ppm_dump(params(4), lights, k)
        assert radius == dmp["radius"] and length == len(dmp["center"])
        want, _ = g.ppm_render(params(k + 1), lights)
        assert image.shape == (h, w, 3) and np.array_equal(image.view(np.uint64), want.view(np.uint64)), k
    assert np.array_equal(seen[3][3].view(np.uint64), img.view(np.uint64))
    assert sum(a[2] for a in seen) == st["photons_stored"]
    o_img, _ = o.ppm_render(params(4), lights)
    assert np.array_equal(img.view(np.uint64), o_img.view(np.uint64))

    class Stop(Exception):
        pass

    def boom(*a):
        raise Stop()

    with pytest.raises(Stop):
        g.ppm_render(params(2), lights, callback=boom)
    again, _ = g.ppm_render(params(4), lights)
    assert np.array_equal(again.view(np.uint64), img.view(np.uint64))
    g.close()


# ---- edges of the argument space ----
@pytest.mark.parametrize("max_bounces", [1, 60])
def test_ppm_shortest_and_longest_paths(P, oracle, max_bounces):
    from path_tracer_ocaml_amd import abi
    w = h = 16
    d = oracle.desc_cornell(w, h, 0.0)
    _check(P, oracle, d, oracle.lights_cornell(w, h), abi.ppm_params(w, h, iterations=2, photon_count=600, max_bounces=max_bounces))


@pytest.mark.parametrize("w,h", [(1, 1), (1, 257), (257, 1)])
def test_ppm_degenerate_images(P, oracle, w, h):
    from path_tracer_ocaml_amd import abi
    d = oracle.desc_cornell(w, h, 0.0)
    _check(P, oracle, d, oracle.lights_cornell(w, h), abi.ppm_params(w, h, iterations=2, photon_count=500))


@pytest.mark.parametrize("alpha", [0.0, 1.0])
def test_ppm_alpha_at_both_ends(P, oracle, alpha):
    from path_tracer_ocaml_amd import abi
    w = h = 20
    d = oracle.desc_cornell(w, h, 0.0)
    _, st = _check(P, oracle, d, oracle.lights_cornell(w, h), abi.ppm_params(w, h, iterations=3, photon_count=1000, alpha=alpha))


def _spot(position, direction, power=5.0):
    from path_tracer_ocaml_amd import abi
    l = abi.Light()
    l.kind = abi.PTX_LIGHT_SPOT
    l.position[:] = list(position)
    l.direction[:] = list(direction)
    l.color[:] = [1.0, 0.8, 0.6]
    l.power = power
    return l


def test_ppm_spot_light_along_plus_z(P, oracle):
    """The other pole branch of Shader_space.create (the shipped scenes only have a spot along -z)."""
    from path_tracer_ocaml_amd import abi
    w = h = 20
    d = oracle.desc_cornell(w, h, 0.0)
    pos = list(oracle.lights_cornell(w, h)[0].position)
    _check(P, oracle, d, [_spot(pos, (0.0, 0.0, 1.0))], abi.ppm_params(w, h, iterations=2, photon_count=1500))


def test_ppm_light_whose_share_truncates_to_no_photon(P, oracle):
    from path_tracer_ocaml_amd import abi
    w = h = 20
    d = oracle.desc_cornell(w, h, 0.0)
    a = oracle.lights_cornell(w, h)[0]
    pos = list(a.position)
    tiny = _spot(pos, (0.0, -1.0, 0.0), power=1e-6)  # 1000 * 1e-6 / (total) truncates to 0: first[] has two equal entries
    _, st = _check(P, oracle, d, [a, tiny, _spot(pos, (0.0, -1.0, 0.2), power=1.0)], abi.ppm_params(w, h, iterations=2, photon_count=1000))


def test_ppm_does_not_read_the_lighting_mode(P, oracle):
    """include/ptx.h: the lighting mode is read by the path integrator's entry points and not by ptx_ppm_render."""
    from path_tracer_ocaml_amd import abi
    w = h = 20
    d = oracle.desc_cornell(w, h, 12.0)  # an emissive ceiling, so that "sampled" can be set
    lights, p = oracle.lights_cornell(w, h), abi.ppm_params(w, h, iterations=2, photon_count=1500)
    o_img, o_st = oracle.Scene(d.ptr, d).ppm_render(p, lights)
    g = P.Scene(d.ptr, 0, keepalive=d)
    img0, st0 = g.ppm_render(p, lights)
    g.set_lighting("sampled")
    assert g.lighting()[0] == abi.PTX_LIGHTING_SAMPLED
    img2, st2 = g.ppm_render(p, lights)
    for img, st in ((img0, st0), (img2, st2)):
        assert np.array_equal(img.view(np.uint64), o_img.view(np.uint64))
        assert all(st[k] == o_st[k] for k in o_st)
    g.close()


def test_ppm_specular_chains_and_a_small_radius(P, oracle):
    """test_ppm_oracle.py's "specular" case: the walk of the photon tree prunes nearly everything."""
    run = R.run_case(oracle, "specular")
    g = P.Scene(run["desc"].ptr, 0, keepalive=run["desc"])
    img, st = g.ppm_render(run["params"], run["lights"])
    assert all(st[k] == run["stats"][k] for k in run["stats"])
    assert np.array_equal(img.view(np.uint64), run["img"].view(np.uint64))
    g.close()


def test_ppm_no_photon_stored(P, oracle):
    """A spot light outside the box that faces away stores nothing: PTX_ERR_STATE (-3) where the oracle gives -2, and the scene
    renders exactly afterwards."""
    from path_tracer_ocaml_amd import abi
    w = h = 16
    d = oracle.desc_cornell(w, h, 0.0)
    away = [_spot((0.0, 0.0, -50.0), (0.0, 0.0, -1.0))]
    p = abi.ppm_params(w, h, iterations=1, photon_count=300)
    with pytest.raises(RuntimeError, match="-2"):
        oracle.Scene(d.ptr, d).ppm_render(p, away)
    g = P.Scene(d.ptr, 0, keepalive=d)
    for env in (None, "1"):
        with pytest.MonkeyPatch.context() as mp:
            if env:
                mp.setenv("PTX_PPM_HOST_LIST", env)
            with pytest.raises(P.PtxError, match=r"\(-3\).*BUG: no photons"):
                g.ppm_render(p, away)
    lights = oracle.lights_cornell(w, h)
    o_img, o_st = oracle.Scene(d.ptr, d).ppm_render(p, lights)
    g_img, g_st = g.ppm_render(p, lights)
    assert np.array_equal(g_img.view(np.uint64), o_img.view(np.uint64)) and all(g_st[k] == o_st[k] for k in o_st)
    g.close()


def test_ppm_gpu_image_inside_the_brute_force_enclosure(P, oracle):
    """The GPU's own image against tests/ppm_reference.py, not only through the oracle: every lit pixel without an undecided pair
    within the reference's bound, every pixel without a neighbour exactly 0, the neighbour total inside its enclosure."""
    run = R.run_case(oracle, "cornell")
    g = P.Scene(run["desc"].ptr, 0, keepalive=run["desc"])
    img, st = g.ppm_render(run["params"], run["lights"])
    g.close()
    ref, bnd, clean, dark = run["frame"]
    n_in = sum(int(x["inside"].sum()) for x in run["gathers"])
    n_und = sum(int(x["undecided"].sum()) for x in run["gathers"])
    assert n_in <= st["neighbors"] <= n_in + n_und
    assert st["photons_stored"] == sum(len(x["center"]) for x in run["dumps"])
    lit = ((ref > 0) | (img > 0)).any(axis=2)
    assert (lit & ~clean).sum() <= 0.01 * lit.sum()
    use = (lit & clean)[:, :, None] & np.ones(3, dtype=bool)
    err = np.abs(img.astype(R.LD) - ref)
    pos = use & (bnd > 0)
    print(f"GPU vs brute force: worst error / bound {float((err[pos] / bnd[pos]).max()):.3f} over {int((lit & clean).sum())} pixels")
    assert use.any() and (err[use] <= bnd[use]).all()
    assert (img[dark] == 0.0).all()


def test_cornell_box_cli(P, tmp_path):
    """cornell-box's Stdlib.Arg command line and prints, PNG rewritten after every iteration."""
    import os
    import subprocess
    from PIL import Image
    from path_tracer_ocaml_amd import abi, host as H
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = os.path.join(root, "path_tracer_ocaml_amd", "cornell_box")
    out = str(tmp_path / "c.png")
    env = dict(os.environ)
    env["LD_LIBRARY_PATH"] = "/opt/rocm/lib:" + env.get("LD_LIBRARY_PATH", "")
    res = subprocess.run([exe, "-width", "96", "-iterations", "2", "-photon-count", "8000", "-o", out], capture_output=True,
                         text=True, env=env, timeout=300)
    assert res.returncode == 0, res.stderr
    for needle in ("#max-bounces = 4", "#photons/iter = 8000", "#iterations = 2", "-----", "#iteration = 1, radius = ",
                   "  photon map length = ", "render time = "):
        assert needle in res.stdout, res.stdout
    hs = H.cornell_box(96, 96, 0.0)
    hs.d.background.kind = abi.PTX_BG_BLACK
    img, _ = P.Scene(hs.ptr, 0, keepalive=hs).ppm_render(abi.ppm_params(96, 96, iterations=2, photon_count=8000), H.lights_cornell(96, 96))
    want = np.clip(H.ppm_gamma(img, 2) * 255.0, 0, 255).astype(np.uint8)
    got = np.array(Image.open(out).convert("RGB"))
    assert np.array_equal(got, want)
    assert subprocess.run([exe, "-bogus"], capture_output=True, env=env).returncode == 2
