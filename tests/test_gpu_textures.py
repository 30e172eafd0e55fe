"""Image textures and the environment on the GPU, bit for bit.

* The rule itself: ptx_texture_eval / ptx_environment_eval (the device's own evaluation functions on explicit inputs) against the
  numpy restatement tests/texture_reference.py, up to PTX_IMAGE_MAX_SIZE texels and indices beyond 2^32.
* Checker equivalence through the whole path: a checker of EVEN cell counts and the image whose texels repeat it (nearest, repeat on
  both axes) trace the same samples -- against the CPU oracle on the checker scene, against the GPU's own checker render, with
  PTX_FUSED=0 and under count_work with the work counters equal -- on Shirley's ground (tree in LDS, Simd_leaf), cornell's wall
  (triangles in LDS) and the floor of a mesh walked from HBM / L2.  Restoring the descriptor's texture restores the old schedule.
* The environment: depth 1 against the restated colour of every camera ray, depth 8 against tests/c/texture_oracle.c, an all-zero
  environment against PTX_BG_BLACK.
* Composition: the feature pass's albedo, progressive = plain, two replicas = one, sampled lighting on an image wall.
Non-periodic images along whole paths are in test_gpu_texture_paths.py."""
import ctypes as C

import numpy as np
import pytest

import texture_reference as T
import texture_support as S

pytestmark = pytest.mark.gpu
W, H, SPP, DEPTH = 64, 32, 4, 8
bits = S.bits


@pytest.fixture(scope="module")
def P():
    import path_tracer_ocaml_amd as P
    assert P.lib().ptx_device_count() >= 1, P.last_error()
    return P


@pytest.fixture(scope="module")
def torch():
    return pytest.importorskip("torch")


# ---------------------------------------------------------------------------------------------------------------- the rule itself
SIZES = [(1, 1), (1, 2), (2, 1), (2, 2), (3, 5), (10, 20)]


def rule_coords(Wt, Ht):
    u, v = T.edge_coordinates(Wt, Ht, np.random.default_rng(Wt * 31 + Ht), 1000)
    extra = np.array([1e6, -1e6, np.nan, 2.0 ** 62, -2.0 ** 62, 2.0 ** 61 / max(Wt, Ht), np.inf, 0.25, -0.0, 1.0])
    eu, ev = np.meshgrid(extra, extra, indexing="ij")
    return np.concatenate([u, eu.ravel()]), np.concatenate([v, ev.ravel()])


@pytest.fixture(scope="module")
def cornell(P, oracle):
    d = oracle.desc_cornell(W, W)
    g = P.Scene(d.ptr, 0, keepalive=d)
    yield g, d
    g.close()


@pytest.mark.parametrize("Wt,Ht", SIZES)
def test_texture_eval_is_the_rule(P, cornell, Wt, Ht):
    """both filters, all four wrap combinations; on a texture entry declared solid (0) and on the checker entry (4)"""
    g, d = cornell
    img = np.random.default_rng(Wt * 7 + Ht).uniform(0.0, 4.0, (Ht, Wt, 3))
    u, v = rule_coords(Wt, Ht)
    uv = np.stack([u, v], axis=1)
    for index in (0, 4):
        for bilinear in (False, True):
            for ru in (False, True):
                for rv in (False, True):
                    g.set_texture_image(index, img, bilinear=bilinear, repeat=(ru, rv))
                    flags = (T.BILINEAR if bilinear else 0) | (T.REPEAT_U if ru else 0) | (T.REPEAT_V if rv else 0)
                    assert g.texture_image(index) == (Wt, Ht, flags)
                    got = g.texture_eval(index, uv)
                    assert np.array_equal(bits(got), bits(T.image_eval(img, flags, u, v))), (index, flags)
        g.set_texture_image(index, None)


@pytest.mark.parametrize("Wt,Ht", T.LIMIT_SIZES)
def test_texture_eval_is_the_rule_at_the_size_limit(P, cornell, Wt, Ht):
    """axes of up to PTX_IMAGE_MAX_SIZE texels and indices that leave 32 bits (the wrap's branch for |i| >= 2^32, whose products are
    largest for n near 16384): both filters, all four wrap combinations.  T.limit_case asserts that the coordinates reach there."""
    g, d = cornell
    img, u, v = T.limit_case(Wt, Ht)
    uv = np.stack([u, v], axis=1)
    try:
        for bilinear in (False, True):
            for ru in (False, True):
                for rv in (False, True):
                    g.set_texture_image(4, img, bilinear=bilinear, repeat=(ru, rv))
                    flags = (T.BILINEAR if bilinear else 0) | (T.REPEAT_U if ru else 0) | (T.REPEAT_V if rv else 0)
                    assert g.texture_image(4) == (Wt, Ht, flags)
                    got = g.texture_eval(4, uv)
                    assert np.array_equal(bits(got), bits(T.image_eval(img, flags, u, v))), flags
    finally:
        g.set_texture_image(4, None)


def test_texture_eval_without_an_image_is_the_descriptors_texture(P, cornell):
    g, d = cornell
    u, v = T.edge_coordinates(10, 10, np.random.default_rng(5), 2000)
    uv = np.stack([u, v], axis=1)
    tex = d.arrays()["textures"]
    assert tex[4][0] == 1 and tex[0][0] == 0
    assert np.array_equal(g.texture_eval(0, uv), np.broadcast_to(tex[0][3:6], (len(uv), 3)))
    wc, hc = int(tex[4][1]) - 1, int(tex[4][2]) - 1
    want = np.where(T.checker_parity(wc, hc, u, v)[:, None] == 0, tex[4][3:6], tex[4][6:9])
    assert np.array_equal(bits(g.texture_eval(4, uv)), bits(want))


def env_directions(n, seed=11):
    rng = np.random.default_rng(seed)
    d = rng.normal(size=(n, 3)) * rng.uniform(0.01, 100.0, (n, 1))
    special = [[0, 1, 0], [0, -1, 0], [1, 0, 0], [-1, 0, 0], [0, 0, 1], [0, 0, -1], [-1, 0, 1e-300], [-1, 0, -1e-300], [-1, 1e-9, 0.0],
               [-1, 0, -0.0], [1e-200, 1, 1e-200], [3, 4, 0], [0, 3, 4], [-2, 0, 2], [-1, 1e-17, 1e-17], [1, 1, 1]]
    d[:len(special)] = special
    k = len(special)
    t = np.linspace(-1e-6, 1e-6, 200)
    d[k:k + 200] = np.stack([-np.ones(200), rng.uniform(-1, 1, 200), t], axis=1)  # the atan2 seam
    d[k + 200:k + 400] = np.stack([t, np.where(np.arange(200) % 2 == 0, 1.0, -1.0), t[::-1]], axis=1)  # the poles
    return d


@pytest.mark.parametrize("bilinear", [False, True])
def test_environment_eval_is_the_rule(P, oracle, cornell, bilinear):
    g, _ = cornell
    env = S.random_environment(16, 8, 5)
    d = env_directions(1 << 16)
    flags = T.BILINEAR if bilinear else 0
    for R in (None, S.rotation([1.0, 2.0, -0.5], 37.0)):
        g.set_environment(env, rotation=R, bilinear=bilinear)
        got = g.environment_eval(d)
        assert np.array_equal(bits(got), bits(T.environment_eval(env, flags, R, d))), R is None
    g.set_environment(None)
    assert np.array_equal(g.environment_eval(d[:100]), np.zeros((100, 3)))  # cornell's own background: black


# ------------------------------------------------------------------------------------------------------------ checker equivalence
def equivalence_case(name, oracle):
    """(descriptor with the even checker, keepalive, texture index, cells (W, H), frame width, height)"""
    return S.equivalence_case(name, oracle, W, H)


def raw_sums(P, torch, g, w, h, **kw):
    raw = torch.zeros((h, w, 3), dtype=torch.float64, device="cuda:0")
    st = g.render_raw_device(P.render_params(w, h, SPP, DEPTH, **kw), raw.data_ptr())
    return raw.cpu().numpy(), st


COUNTERS = ("segments", "nodes_tested", "prims_tested", "floor_tested")


@pytest.mark.parametrize("name", ["shirley", "cornell", "mesh"])
def test_checker_image_equals_the_checker(P, torch, oracle, name, monkeypatch):
    d, keep, index, (cw, ch), w, h = equivalence_case(name, oracle)
    ptr = C.pointer(d)
    xs, ys, ps = S.all_samples(w, h, SPP)
    o_scene = oracle.Scene(ptr, keep)
    want, _ = o_scene.trace_samples(w, h, SPP, DEPTH, xs, ys, ps)
    o_scene.close()
    even, odd = S.checker_colours(d, index)
    img = T.checker_image(cw, ch, even, odd)
    for fused in ("2", "0"):
        monkeypatch.setenv("PTX_FUSED", fused)
        chk, g = P.Scene(ptr, 0, keepalive=keep), P.Scene(ptr, 0, keepalive=keep)
        try:
            assert g.stats()["traversal_in_lds"] == (0 if name == "mesh" else 1)
            plain_raw, plain_st = raw_sums(P, torch, g, w, h, count_work=True)  # the schedule before any image
            g.set_texture_image(index, img, repeat=(True, True))
            got, _ = g.trace_samples(w, h, SPP, DEPTH, xs, ys, ps)
            assert np.array_equal(bits(got), bits(want)), fused  # the oracle on the CHECKER scene, no sample excluded
            got_chk, _ = chk.trace_samples(w, h, SPP, DEPTH, xs, ys, ps)
            assert np.array_equal(bits(got_chk), bits(want)), fused
            raw_chk, _ = raw_sums(P, torch, chk, w, h)
            raw_img, st = raw_sums(P, torch, g, w, h)
            assert np.array_equal(bits(raw_img), bits(raw_chk)), fused
            assert st["carry_launches"] == 0 and st["lds_oct_launches"] == 0
            # counting: the same sums and the same work
            raw_chk_c, st_chk = raw_sums(P, torch, chk, w, h, count_work=True)
            raw_img_c, st_img = raw_sums(P, torch, g, w, h, count_work=True)
            assert np.array_equal(bits(raw_img_c), bits(raw_chk)) and np.array_equal(bits(raw_chk_c), bits(raw_chk)), fused
            for k in COUNTERS:
                assert st_img[k] == st_chk[k], k
            assert st_img["segments"] > 0 and st_img["nodes_tested"] > 0
            assert st_img["carry_launches"] == 0 and st_img["solo_launches"] == 0
            _, st_t = g.trace_samples(w, h, SPP, DEPTH, xs, ys, ps, count_work=True)
            _, st_tc = chk.trace_samples(w, h, SPP, DEPTH, xs, ys, ps, count_work=True)
            assert [st_t[k] for k in COUNTERS] == [st_tc[k] for k in COUNTERS]
            # the descriptor's texture again: the old schedule again
            g.set_texture_image(index, None)
            assert g.texture_image(index) is None
            back_raw, back_st = raw_sums(P, torch, g, w, h, count_work=True)
            assert np.array_equal(bits(back_raw), bits(plain_raw))
            assert back_st["carry_launches"] == plain_st["carry_launches"] == st_chk["carry_launches"]
            if name == "shirley" and fused == "2":
                assert back_st["carry_launches"] > 0  # Shirley's default is the shade-first order
                _, st_nc = raw_sums(P, torch, g, w, h)
                assert st_nc["lds_oct_launches"] > 0
        finally:
            chk.close()
            g.close()


def test_an_image_on_a_solid_entry_gives_its_slots_tex_coords(P, torch, oracle):
    """cornell's white walls are declared solid: their slots compute no tex coords until the entry carries an image.  A one-texel image
    of the same colour is that solid; a two-colour one is not."""
    d = oracle.desc_cornell(W, H)
    tex = d.arrays()["textures"]
    index = 3
    assert tex[index][0] == 0
    g = P.Scene(d.ptr, 0, keepalive=d)
    plain, _ = raw_sums(P, torch, g, W, H)
    g.set_texture_image(index, tex[index][3:6].reshape(1, 1, 3))
    same, _ = raw_sums(P, torch, g, W, H)
    assert np.array_equal(bits(same), bits(plain))
    g.set_texture_image(index, T.checker_image(4, 4, [0.7, 0.1, 0.1], [0.1, 0.1, 0.7]), repeat=(True, True))
    other, _ = raw_sums(P, torch, g, W, H)
    assert not np.array_equal(other, plain)
    g.close()


# -------------------------------------------------------------------------------------------------------------------- environment
@pytest.mark.parametrize("bilinear", [False, True])
def test_environment_depth_one(P, oracle, bilinear):
    """every miss's radiance is the restated colour of its camera ray, every hit is 0"""
    d = oracle.desc_shirley(W, H)
    env = S.random_environment(32, 16, 9)
    R = S.rotation([0.3, 1.0, 0.2], 120.0)
    xs, ys, ps = S.all_samples(W, H, SPP)
    o, dirs = S.camera_rays(oracle, d.d, W, H, SPP, 1, xs, ys, ps)
    o_scene = oracle.Scene(d.ptr, d)
    _, prim, _ = o_scene.intersect_rays(o, dirs)
    o_scene.close()
    miss = prim < 0
    assert 0.1 < miss.mean() < 0.9
    flags = T.BILINEAR if bilinear else 0
    want = np.where(miss[:, None], T.environment_eval(env, flags, R, dirs), 0.0) + 0.0
    g = P.Scene(d.ptr, 0, keepalive=d)
    g.set_environment(env, rotation=R, bilinear=bilinear)
    got, _ = g.trace_samples(W, H, SPP, 1, xs, ys, ps)
    g.close()
    assert np.array_equal(bits(got), bits(want))


@pytest.mark.parametrize("name", ["shirley", "mesh"])
def test_environment_depth_eight(P, torch, oracle, name, monkeypatch):
    d = oracle.desc_shirley(W, H) if name == "shirley" else oracle.desc_ganesha_like(W, H, n_target=6000)
    env = S.random_environment(32, 16, 21)
    R = S.rotation([0.0, 1.0, 0.0], 75.0)
    xs, ys, ps = S.all_samples(W, H, SPP)
    ref = S.Restatement(d.ptr, d)
    want = ref.trace_samples(env, T.BILINEAR, R, W, H, SPP, DEPTH, xs, ys, ps)
    ref.close()
    for fused in ("2", "0"):
        monkeypatch.setenv("PTX_FUSED", fused)
        g = P.Scene(d.ptr, 0, keepalive=d)
        g.set_environment(env, rotation=R)
        got, _ = g.trace_samples(W, H, SPP, DEPTH, xs, ys, ps)
        assert np.array_equal(bits(got), bits(want)), fused
        raw, st = raw_sums(P, torch, g, W, H)
        sums = np.zeros((H * W, 3))
        for p in range(SPP):  # pass order, from zero
            sums = sums + want.reshape(H * W, SPP, 3)[:, p]
        assert np.array_equal(bits(raw), bits(sums.reshape(H, W, 3))), fused
        assert st["carry_launches"] == 0 and st["lds_oct_launches"] == 0
        g.close()


def test_an_all_zero_environment_is_a_black_background(P, torch, oracle):
    src = oracle.desc_shirley(W, H)
    d = S.abi.SceneDesc()
    C.memmove(C.byref(d), C.byref(src.d), C.sizeof(S.abi.SceneDesc))
    d.background.kind = 0  # PTX_BG_BLACK
    black = P.Scene(C.pointer(d), 0, keepalive=(d, src))
    g = P.Scene(src.ptr, 0, keepalive=src)
    g.set_environment(np.zeros((4, 8, 3)))
    a, _ = raw_sums(P, torch, black, W, H)
    b, _ = raw_sums(P, torch, g, W, H)
    assert np.array_equal(bits(a), bits(b)) and not a.any()  # Shirley's scene has no emitter: all light was the sky's
    black.close()
    g.close()


# -------------------------------------------------------------------------------------------------------------------- composition
def test_feature_albedo_is_the_bilinear_texel(P, torch, oracle):
    """first hits on cornell's image-textured wall: the tex coords from the oracle's Triangle.intersect of the oracle's camera ray,
    combined as Triangle.Hit.to_hit combines them"""
    w = h = 48
    d = oracle.desc_cornell(w, h)
    a = d.arrays()
    index = 4
    img = np.random.default_rng(4).uniform(0.0, 1.0, (7, 5, 3))
    g = P.Scene(d.ptr, 0, keepalive=d)
    g.set_texture_image(index, img, bilinear=True, repeat=(False, True))
    feat = torch.zeros((h, w, 8), dtype=torch.float64, device="cuda:0")
    g.render_features_device(P.render_params(w, h, SPP, 2), 1, 1, feat.data_ptr())  # pass 1 alone
    feat = feat.cpu().numpy().reshape(h * w, 8)
    ys, xs = np.mgrid[0:h, 0:w]
    xs, ys = xs.ravel(), ys.ravel()
    o, dirs = S.camera_rays(oracle, d.d, w, h, SPP, 2, xs, ys, np.ones(h * w, dtype=np.int64))
    o_scene = oracle.Scene(d.ptr, d)
    _, prim, _ = o_scene.intersect_rays(o, dirs)
    o_scene.close()
    n_tri = len(a["tri_material"])
    tex_of = np.array([int(a["materials"][m][1]) if a["materials"][m][0] != 2 else -1 for m in a["tri_material"]])
    on_wall = (prim >= 0) & (prim < n_tri)
    on_wall[on_wall] = tex_of[prim[on_wall]] == index
    assert on_wall.sum() > 100
    L = oracle.lib()
    tuv = np.zeros(3)
    want_rows, rows = [], np.flatnonzero(on_wall)
    tu, tv = np.zeros(len(rows)), np.zeros(len(rows))
    for k, i in enumerate(rows):
        t = int(prim[i])
        idx = a["tri_indices"][3 * t:3 * t + 3]
        abc = S.f64([[a["vertex_x"][j], a["vertex_y"][j], a["vertex_z"][j]] for j in idx]).reshape(-1)
        assert L.orc_triangle_intersect(S._dp(abc), S._dp(S.f64(o[i])), S._dp(S.f64(dirs[i])), 0.0, 1.7976931348623157e308, S._dp(tuv))
        u, v = tuv[1], tuv[2]
        wgt = 1.0 - u - v
        uv = a["tri_uv"][6 * t:6 * t + 6]
        tu[k] = (uv[0] * wgt) + (uv[2] * u) + (uv[4] * v)
        tv[k] = (uv[1] * wgt) + (uv[3] * u) + (uv[5] * v)
    want = T.image_eval(img, T.BILINEAR | T.REPEAT_V, tu, tv)
    assert np.array_equal(bits(feat[rows, 0:3]), bits(want))
    assert (feat[rows, 7] == 1.0).all()
    g.close()


def test_feature_albedo_of_a_miss_is_the_environment(P, torch, oracle):
    d = oracle.desc_shirley(W, H)
    env = S.random_environment(16, 8, 2)
    g = P.Scene(d.ptr, 0, keepalive=d)
    g.set_environment(env)
    feat = torch.zeros((H, W, 8), dtype=torch.float64, device="cuda:0")
    g.render_features_device(P.render_params(W, H, SPP, 2), 0, 1, feat.data_ptr())
    feat = feat.cpu().numpy().reshape(H * W, 8)
    ys, xs = np.mgrid[0:H, 0:W]
    o, dirs = S.camera_rays(oracle, d.d, W, H, SPP, 2, xs.ravel(), ys.ravel(), np.zeros(H * W, dtype=np.int64))
    miss = feat[:, 7] == 0.0
    assert 0.1 < miss.mean() < 0.9
    assert np.array_equal(bits(feat[miss, 0:3]), bits(T.environment_eval(env, T.BILINEAR, None, dirs[miss])))
    g.close()


def test_progressive_and_two_replicas_give_the_plain_image(P, oracle, monkeypatch):
    d, keep = S.with_checker(oracle.desc_shirley(W, H), 0, 11, 21)
    g = P.Scene(C.pointer(d), 0, keepalive=keep)
    g.set_texture_image(0, np.random.default_rng(8).uniform(0.0, 1.0, (9, 6, 3)), bilinear=True, repeat=(True, True))
    g.set_environment(S.random_environment(32, 16, 3), rotation=S.rotation([0, 1, 0], 30.0))
    plain, _ = g.render(W, H, SPP, DEPTH)
    assert plain.max() > 0.5
    prog, _, done, _ = g.render_progressive(W, H, SPP, DEPTH, 1)
    assert done == SPP and np.array_equal(bits(prog), bits(plain))
    monkeypatch.setenv("PTX_MULTI_ALIAS", "1")  # test hook: replicas may share a device
    two, _ = g.render(W, H, SPP, DEPTH, n_gpus=2)
    assert np.array_equal(bits(two), bits(plain))
    # replicas follow the root scene: a change after they exist reaches them
    g.set_environment(None)
    g.set_texture_image(0, None)
    one, _ = g.render(W, H, SPP, DEPTH)
    two, _ = g.render(W, H, SPP, DEPTH, n_gpus=2)
    assert np.array_equal(bits(two), bits(one)) and not np.array_equal(one, plain)
    r = g.replicate(0)
    g.set_environment(S.random_environment(8, 4, 1))
    r2 = g.replicate(0)  # ptx_scene_replicate copies the state
    assert r.environment() is None and r2.environment()[0] == (8, 4, 1)
    r.close()
    r2.close()
    g.close()


def test_sampled_lighting_on_an_image_wall(P, oracle):
    """lighting mode 2 on cornell whose checker wall is an image: mode 2's own restatement on the equivalent checker"""
    import lighting_support as LS
    w = h = 32
    d, keep = S.with_checker(oracle.desc_cornell(w, h), 4, 11, 11)
    ptr = C.pointer(d)
    xs, ys, ps = S.all_samples(w, h, SPP)
    ref = LS.Restatement(ptr, keep)
    want = ref.trace_samples(2, w, h, SPP, DEPTH, xs, ys, ps)
    ref.close()
    even, odd = S.checker_colours(d, 4)
    g = P.Scene(ptr, 0, keepalive=keep)
    g.set_lighting("sampled")
    g.set_texture_image(4, T.checker_image(10, 10, even, odd), repeat=(True, True))
    got, _ = g.trace_samples(w, h, SPP, DEPTH, xs, ys, ps)
    g.close()
    assert np.array_equal(bits(got), bits(want))


def test_cli_envmap_and_ground_texture(P, tmp_path):
    """shirley_spheres --envmap --envmap-rotate --ground-texture --texture-nearest writes the PNG the same calls give through Python"""
    import os
    import subprocess
    from path_tracer_ocaml_amd import host
    from test_pfm import write_pfm
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    rng = np.random.default_rng(6)
    env = rng.uniform(0.0, 2.0, (8, 16, 3)).astype(np.float32)
    tex = rng.uniform(0.0, 1.0, (6, 4)).astype(np.float32)  # a grey file
    write_pfm(tmp_path / "env.pfm", env, little=False)
    write_pfm(tmp_path / "tex.pfm", tex)
    w, h, spp = 96, 48, 4
    R = (C.c_double * 9)()
    host.lib().pth_rotation_y.argtypes = [C.c_double, C.POINTER(C.c_double)]
    host.lib().pth_rotation_y(40.0, R)
    hs = host.shirley_spheres(w, h)
    g = P.Scene(hs.ptr, 0, keepalive=hs)
    g.set_environment(env.astype(np.float64), rotation=np.array(list(R)))
    g.set_texture_image(0, np.repeat(tex.astype(np.float64)[:, :, None], 3, axis=2), repeat=(True, True))
    want, _ = g.render(w, h, spp, 8)
    g.close()
    host.write_png(str(tmp_path / "want.png"), want)
    out = tmp_path / "got.png"
    r = subprocess.run([os.path.join(root, "path_tracer_ocaml_amd", "shirley_spheres"), f"--dimension={w},{h}", f"--samples-per-pixel={spp}",
                        "--no-progress", f"--envmap={tmp_path / 'env.pfm'}", "--envmap-rotate=40", f"--ground-texture={tmp_path / 'tex.pfm'}",
                        "--texture-nearest", "-o", str(out)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert out.read_bytes() == (tmp_path / "want.png").read_bytes()
    r = subprocess.run([os.path.join(root, "path_tracer_ocaml_amd", "shirley_spheres"), f"--dimension={w},{h}",
                        f"--envmap={tmp_path / 'missing.pfm'}"], capture_output=True, text=True)
    assert r.returncode == 1 and "cannot open" in r.stderr


@pytest.mark.parametrize("threads", ["1024", "768", "64"])
def test_image_kernels_at_any_workgroup_size(P, torch, oracle, threads, monkeypatch):
    """the IMG instantiations are compiled for 3 waves per SIMD, i.e. at most 768 threads a workgroup: a larger PTX_BOUNCE_THREADS is
    clamped for a scene with an image (and only for it), and every size renders the checker's bits"""
    d, keep, index, (cw, ch), w, h = equivalence_case("shirley", oracle)
    ptr = C.pointer(d)
    even, odd = S.checker_colours(d, index)
    monkeypatch.setenv("PTX_BOUNCE_THREADS", threads)
    chk, g = P.Scene(ptr, 0, keepalive=keep), P.Scene(ptr, 0, keepalive=keep)
    g.set_texture_image(index, T.checker_image(cw, ch, even, odd), bilinear=False, repeat=(True, True))
    g.set_environment(np.zeros((2, 4, 3)))
    a, _ = raw_sums(P, torch, chk, w, h)
    # (an all-zero environment under Shirley's sky differs from the sky: compare against the same environment on the checker scene)
    chk.set_environment(np.zeros((2, 4, 3)))
    b, _ = raw_sums(P, torch, chk, w, h)
    c, _ = raw_sums(P, torch, g, w, h)
    assert a.any() and np.array_equal(bits(b), bits(c))
    chk.close()
    g.close()
