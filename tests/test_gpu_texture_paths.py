"""Image textures along whole paths on the GPU, bit for bit against tests/c/texture_oracle.c's image-table tracer.

The images are seeded noise of sizes with W != H that are no powers of two, several per scene and all set at once, bilinear and
nearest, every wrap combination, on Lambertian, metal and emitting materials, on spheres small and large (the atan2 seam included),
on triangles in LDS and on mesh triangles walked from HBM, with and without an environment: texture_support.path_case.  That each
way of getting the lookup wrong changes these frames, and that every imaged entry is seen directly, is checked without a GPU in
test_texture_reference.py.

* every sample of a 64 x 32 frame at 4 spp, depth 8: ptx_trace_samples = the restatement, the raw sums = its samples added in pass
  order, under PTX_FUSED=2 and 0, with and without count_work, the work counters the oracle's on the scene without images;
* workgroup sizes 64 and 1024; the feature pass's albedo and hit flag on every pixel; setting, replacing and removing images in
  several orders; a replica made after the images were set."""
import numpy as np
import pytest

import texture_support as S

pytestmark = pytest.mark.gpu
W, H, SPP, DEPTH = S.PATH_W, S.PATH_H, S.PATH_SPP, S.PATH_DEPTH
bits = S.bits
COUNTERS = ("segments", "nodes_tested", "prims_tested", "floor_tested")
_REF = {}


@pytest.fixture(scope="module")
def P():
    import path_tracer_ocaml_amd as P
    assert P.lib().ptx_device_count() >= 1, P.last_error()
    return P


@pytest.fixture(scope="module")
def torch():
    return pytest.importorskip("torch")


def env_kw(case, with_env):
    return dict(zip(("env", "env_flags", "R"), case["env"])) if with_env else {}


def reference(oracle, name, with_env, images=None):
    """the restatement's samples and their pass-order sums, the oracle's counters on the scene without images and the first hits of
    pass 1; computed once per (scene, environment, image set) and left unchanged"""
    key = (name, with_env, None if images is None else tuple(sorted((i, im.shape, f) for i, (im, f) in images.items())))
    if key not in _REF:
        case = S.path_case(name, oracle)
        d = case["desc"]
        imgs = case["images"] if images is None else images
        xs, ys, ps = S.all_samples(W, H, SPP)
        ref = S.Restatement(d.ptr, d)
        want = ref.trace_samples_images(imgs, W, H, SPP, DEPTH, xs, ys, ps, **env_kw(case, with_env))
        one = ps == 1
        first = ref.first_hits(imgs, W, H, SPP, DEPTH, xs[one], ys[one], ps[one], **env_kw(case, with_env))
        ref.close()
        o = oracle.Scene(d.ptr, d)
        _, counters = o.trace_samples(W, H, SPP, DEPTH, xs, ys, ps)
        o.close()
        want.setflags(write=False)
        _REF[key] = {"case": case, "images": imgs, "want": want, "sums": S.pass_order_sums(want, W, H, SPP), "counters": counters,
                     "first": first, "with_env": with_env}
    return _REF[key]


def gpu_scene(P, ref, images=None):
    case = ref["case"]
    g = P.Scene(case["desc"].ptr, 0, keepalive=case["desc"])
    S.set_images(g, ref["images"] if images is None else images)
    if ref["with_env"]:
        env, flags, R = case["env"]
        g.set_environment(env, rotation=R, bilinear=bool(flags & S.BILINEAR))
    return g


def raw_sums(P, torch, g, **kw):
    raw = torch.zeros((H, W, 3), dtype=torch.float64, device="cuda:0")
    st = g.render_raw_device(P.render_params(W, H, SPP, DEPTH, **kw), raw.data_ptr())
    return raw.cpu().numpy(), st


def n_differ(got, want):
    return int((bits(got) != bits(want)).any(axis=-1).sum())


def check_paths(P, torch, ref, what):
    xs, ys, ps = S.all_samples(W, H, SPP)
    g = gpu_scene(P, ref)
    try:
        if ref["case"]["lds"] is not None:
            assert g.stats()["traversal_in_lds"] == ref["case"]["lds"]
        got, _ = g.trace_samples(W, H, SPP, DEPTH, xs, ys, ps)
        assert n_differ(got, ref["want"]) == 0, what  # every sample of the frame, none excluded
        raw, st = raw_sums(P, torch, g)
        assert n_differ(raw, ref["sums"]) == 0, what
        assert st["carry_launches"] == 0 and st["lds_oct_launches"] == 0, what
        raw_c, st_c = raw_sums(P, torch, g, count_work=True)
        assert n_differ(raw_c, ref["sums"]) == 0, what
        got_c, st_t = g.trace_samples(W, H, SPP, DEPTH, xs, ys, ps, count_work=True)
        assert n_differ(got_c, ref["want"]) == 0, what
        for k in COUNTERS:  # an image or an environment changes colours and never a path
            assert st_c[k] == ref["counters"][k] and st_t[k] == ref["counters"][k], (what, k, st_c[k], st_t[k], ref["counters"][k])
        assert st_c["carry_launches"] == 0 and st_c["lds_oct_launches"] == 0, what
    finally:
        g.close()


@pytest.mark.parametrize("fused", ["2", "0"])
@pytest.mark.parametrize("name,with_env", [("shirley", False), ("shirley", True), ("cornell", False), ("mesh", True)])
def test_paths_are_the_restatement(P, torch, oracle, name, with_env, fused, monkeypatch):
    """Shirley (Simd_leaf, tree in LDS) under its sky and under a rotated bilinear environment; cornell (triangles in LDS, black
    background, an emitter); the 6000-triangle mesh walked from HBM / L2 under the environment"""
    monkeypatch.setenv("PTX_FUSED", fused)
    check_paths(P, torch, reference(oracle, name, with_env), (name, with_env, fused))


def test_paths_on_array_leaves_are_the_restatement(P, torch, oracle, monkeypatch):
    monkeypatch.setenv("PTX_FUSED", "2")
    check_paths(P, torch, reference(oracle, "shirley_array", False), "shirley_array")


@pytest.mark.parametrize("threads", ["64", "1024"])
def test_paths_at_other_workgroup_sizes(P, torch, oracle, threads, monkeypatch):
    monkeypatch.setenv("PTX_BOUNCE_THREADS", threads)
    ref = reference(oracle, "shirley", False)
    xs, ys, ps = S.all_samples(W, H, SPP)
    g = gpu_scene(P, ref)
    try:
        got, _ = g.trace_samples(W, H, SPP, DEPTH, xs, ys, ps)
        assert n_differ(got, ref["want"]) == 0
        raw, _ = raw_sums(P, torch, g)
        assert n_differ(raw, ref["sums"]) == 0
    finally:
        g.close()


@pytest.mark.parametrize("name,with_env", [("shirley", False), ("shirley", True), ("cornell", False), ("mesh", True)])
def test_feature_pass_is_the_first_hit(P, torch, oracle, name, with_env):
    """pass 1 alone, every pixel: Lambertian and metal show the image colour, a dielectric (1, 1, 1), a miss the background or the
    environment"""
    ref = reference(oracle, name, with_env)
    albedo, hit, tex, _ = ref["first"]
    assert (hit == 0).any() and all((tex == i).any() for i in ref["images"])
    if name != "mesh":
        assert ((hit == 1) & (tex < 0)).any()  # a dielectric
    g = gpu_scene(P, ref)
    try:
        feat = torch.zeros((H, W, 8), dtype=torch.float64, device="cuda:0")
        g.render_features_device(P.render_params(W, H, SPP, DEPTH), 1, 1, feat.data_ptr())
        feat = feat.cpu().numpy().reshape(H * W, 8)
    finally:
        g.close()
    assert n_differ(feat[:, 0:3], albedo) == 0
    assert np.array_equal(feat[:, 7], hit.astype(np.float64))


def test_setting_replacing_and_removing_images(P, torch, oracle):
    """cornell, raw sums: the table of images is the set of (entry, image) pairs, whatever the order it was reached in"""
    case = S.path_case("cornell", oracle)
    d, images = case["desc"], case["images"]
    other = (S.random_image(31, 2, 70), S.BILINEAR | S.REPEAT_V)

    def fresh(entries):
        g = P.Scene(d.ptr, 0, keepalive=d)
        S.set_images(g, entries)
        return g

    def sums_of(entries):
        g = fresh(entries)
        try:
            return raw_sums(P, torch, g)[0]
        finally:
            g.close()

    pick = lambda *idx: {i: images[i] for i in idx}  # noqa: E731 (a dict keeps the order given)
    g, plain = fresh(pick(4, 0, 6)), P.Scene(d.ptr, 0, keepalive=d)
    try:
        plain_raw, plain_st = raw_sums(P, torch, plain)
        three = raw_sums(P, torch, g)[0]
        assert n_differ(three, sums_of(pick(6, 4, 0))) == 0
        assert n_differ(three, reference(oracle, "cornell", False, images=pick(0, 4, 6))["sums"]) == 0
        g.set_texture_image(0, None)  # one of three removed
        two = raw_sums(P, torch, g)[0]
        assert g.texture_image(0) is None and g.texture_image(4) == (7, 5, images[4][1]) and g.texture_image(6) == (2, 2, images[6][1])
        assert n_differ(two, sums_of(pick(4, 6))) == 0 and n_differ(two, three) > 0
        S.set_images(g, {4: other})  # an image of another size in its place
        assert g.texture_image(4) == (31, 2, other[1])
        replaced = raw_sums(P, torch, g)[0]
        assert n_differ(replaced, sums_of({4: other, 6: images[6]})) == 0 and n_differ(replaced, two) > 0
        g.set_texture_image(6, None)
        alone = raw_sums(P, torch, g)[0]
        assert n_differ(alone, sums_of({4: other})) == 0 and n_differ(alone, replaced) > 0
        assert n_differ(alone, reference(oracle, "cornell", False, images={4: other})["sums"]) == 0
        g.set_texture_image(4, None)  # none left: the plain scene and its schedule
        back, back_st = raw_sums(P, torch, g)
        assert n_differ(back, plain_raw) == 0 and n_differ(back, alone) > 0
        assert back_st["carry_launches"] == plain_st["carry_launches"]
        assert all(g.texture_image(i) is None for i in range(d.d.n_textures))
    finally:
        g.close()
        plain.close()


def test_a_replica_made_after_the_images_renders_the_roots_bits(P, torch, oracle, monkeypatch):
    """cornell's whole image set: bilinear noise on both metal entries (0 and 6) among it"""
    ref = reference(oracle, "cornell", False)
    images = ref["images"]
    assert all(images[i][1] & S.BILINEAR for i in (0, 6))
    g = gpu_scene(P, ref)
    try:
        one, _ = g.render(W, H, SPP, DEPTH)
        monkeypatch.setenv("PTX_MULTI_ALIAS", "1")  # test hook: replicas may share a device
        two, _ = g.render(W, H, SPP, DEPTH, n_gpus=2)  # the replicas are made here, after the images
        assert one.max() > 0.0 and np.array_equal(bits(two), bits(one))
        r = g.replicate(0)
        try:
            assert [r.texture_image(i) for i in sorted(images)] == [(images[i][0].shape[1], images[i][0].shape[0], images[i][1])
                                                                    for i in sorted(images)]
            assert n_differ(raw_sums(P, torch, r)[0], ref["sums"]) == 0
        finally:
            r.close()
    finally:
        g.close()
