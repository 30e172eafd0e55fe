"""The numpy restatement of the image rule (tests/texture_reference.py) checks itself, and the C restatement
(tests/c/texture_oracle.c: the oracle's source included unchanged, the rule written out in C from include/ptx.h) agrees with it bit
for bit -- on explicit coordinates (up to the size limit and indices beyond 2^32), on directions, and on a depth-1 frame traced under
an environment.  The image-table tracer is held to the oracle where the two must agree, and the scenes and images of the GPU's
whole-path tests (texture_support.path_case) are shown to tell each way of getting the lookup wrong from the rule.  No GPU."""
import numpy as np
import pytest

import texture_reference as T
import texture_support as S

EVEN, ODD = np.array([0.2, 0.3, 0.1]), np.array([0.9, 0.9, 0.9])
SIZES = [(1, 1), (1, 2), (2, 1), (2, 2), (3, 5), (10, 20)]  # (W, H)
WRAPS = [0, T.REPEAT_U, T.REPEAT_V, T.REPEAT_U | T.REPEAT_V]


def image(W, H, seed=3):
    return np.random.default_rng(seed + 100 * W + H).uniform(0.0, 4.0, (H, W, 3))


def coords(W, H):
    u, v = T.edge_coordinates(W, H, np.random.default_rng(W * 31 + H), 2000)
    extra = np.array([1e6, -1e6, np.nan, 2.0 ** 62, -2.0 ** 62, 2.0 ** 61 / max(W, H), 1e300, np.inf, -np.inf, 0.25])
    eu, ev = np.meshgrid(extra, extra, indexing="ij")
    return np.concatenate([u, eu.ravel()]), np.concatenate([v, ev.ravel()])


@pytest.mark.parametrize("W,H", SIZES)
@pytest.mark.parametrize("wrap", WRAPS)
def test_bilinear_at_a_texel_centre_is_that_texel(W, H, wrap):
    img = image(W, H)
    iy, ix = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    # (ix + 0.5) / W * W - 0.5 is ix exactly for these sizes when the quotient rounds back; take the centres that do
    u, v = (ix.ravel() + 0.5) / W, (iy.ravel() + 0.5) / H
    exact = (u * W - 0.5 == ix.ravel()) & (v * H - 0.5 == iy.ravel())
    assert exact.sum() >= max(1, (W * H) // 2)
    got = T.image_eval(img, T.BILINEAR | wrap, u[exact], v[exact])
    assert np.array_equal(S.bits(got), S.bits(img[iy.ravel()[exact], ix.ravel()[exact]]))


@pytest.mark.parametrize("W,H", [(10, 20), (8, 8), (500, 500)])
def test_nearest_on_the_checker_image_is_the_checker(W, H):
    """even W and H, repeat on both axes: no (u, v) disagrees -- negative, 0, 1, 1 - 2^-53, -0.0, up to +-3"""
    rng = np.random.default_rng(W + H)
    u, v = T.edge_coordinates(min(W, 20), min(H, 20), rng, 100_000)
    if W > 20:  # the edges of the real grid too
        k = rng.integers(-W, 2 * W, 4000)
        u = np.concatenate([u, k / W, np.nextafter(k / W, -10.0), np.nextafter(k / W, 10.0)])
        v = np.concatenate([v, np.resize(v, 3 * len(k))])
    assert len(u) >= 100_000
    got = T.image_eval(T.checker_image(W, H, EVEN, ODD), T.REPEAT_U | T.REPEAT_V, u, v)
    want = np.where(T.checker_parity(W, H, u, v)[:, None] == 0, EVEN, ODD)
    assert np.array_equal(S.bits(got), S.bits(want))


def test_an_odd_width_disagrees_exactly_at_u_equal_one():
    """why the equivalence tests use even sizes: with W = 3, ix = W wraps to texel 0 (even) while the checker sees parity 1"""
    W, H = 3, 4
    u = np.array([1.0, 1.0 - 2.0 ** -53, 0.5])
    v = np.full(3, 0.1)
    got = T.image_eval(T.checker_image(W, H, EVEN, ODD), T.REPEAT_U | T.REPEAT_V, u, v)
    want = np.where(T.checker_parity(W, H, u, v)[:, None] == 0, EVEN, ODD)
    same = (S.bits(got) == S.bits(want)).all(axis=1)
    assert same.tolist() == [False, True, True]


def test_wrap_and_out_of_range_inputs():
    img = image(3, 5)
    corner = lambda x, y: img[y, x]  # noqa: E731
    # clamp: outside coordinates take the edge texel; repeat: they come round
    assert np.array_equal(T.image_eval(img, 0, [-0.2, 1.7, 1e6], [-3.0, 9.0, -1e6]), np.array([corner(0, 0), corner(2, 4), corner(2, 0)]))
    assert np.array_equal(T.image_eval(img, T.REPEAT_U | T.REPEAT_V, [-0.4, 1.7], [1.0, -0.3]), np.array([corner(2, 0), corner(2, 4)]))
    # NaN, and a product that reaches 2^62, evaluate as coordinate 0
    zero = T.image_eval(img, 0, [0.0], [0.0])
    for bad in (np.nan, 2.0 ** 62, -2.0 ** 62, np.inf, 1e300):
        assert np.array_equal(T.image_eval(img, 0, [bad], [bad]), zero), bad
        for flags in (T.BILINEAR, T.BILINEAR | T.REPEAT_U | T.REPEAT_V):
            assert np.array_equal(S.bits(T.image_eval(img, flags, [bad], [0.3])), S.bits(T.image_eval(img, flags, [0.0], [0.3]))), bad
    assert not np.array_equal(T.image_eval(img, 0, [2.0 ** 61 / 3], [0.0]), zero)  # just inside: clamps to the last column


@pytest.mark.parametrize("W,H", SIZES)
@pytest.mark.parametrize("bilinear", [0, T.BILINEAR])
def test_c_restatement_equals_numpy_on_coordinates(W, H, bilinear):
    img = image(W, H)
    u, v = coords(W, H)
    for wrap in WRAPS:
        got = S.c_image_eval(img, bilinear | wrap, u, v)
        assert np.array_equal(S.bits(got), S.bits(T.image_eval(img, bilinear | wrap, u, v))), wrap


def directions(n, seed=11):
    rng = np.random.default_rng(seed)
    d = rng.normal(size=(n, 3)) * rng.uniform(0.01, 100.0, (n, 1))
    special = [[0, 1, 0], [0, -1, 0], [1, 0, 0], [-1, 0, 0], [0, 0, 1], [0, 0, -1], [-1, 0, 1e-300], [-1, 0, -1e-300], [-1, 1e-9, 0.0],
               [-1, 0, -0.0], [1e-200, 1, 1e-200], [3, 4, 0], [0, 3, 4], [-2, 0, 2], [-1, 1e-17, 1e-17], [1, 1, 1]]
    d[:len(special)] = special
    # the atan2 seam (-x axis, z of either sign) and the poles, densely
    k = len(special)
    t = np.linspace(-1e-6, 1e-6, 200)
    d[k:k + 200] = np.stack([-np.ones(200), rng.uniform(-1, 1, 200), t], axis=1)
    d[k + 200:k + 400] = np.stack([t, np.where(np.arange(200) % 2 == 0, 1.0, -1.0), t[::-1]], axis=1)
    return d


@pytest.mark.parametrize("bilinear", [0, T.BILINEAR])
def test_c_restatement_equals_numpy_on_directions(oracle, bilinear):
    env = S.random_environment(16, 8, 5)
    d = directions(1 << 14)
    for R in (None, S.rotation([1.0, 2.0, -0.5], 37.0)):
        got = S.c_environment_eval(env, bilinear, R, d)
        assert np.array_equal(S.bits(got), S.bits(T.environment_eval(env, bilinear, R, d)))
    u, v = T.environment_uv(np.array([[0.0, 1.0, 0.0], [0.0, -1.0, 0.0], [1.0, 0.0, 0.0]]))
    assert v.tolist() == [1.0, 0.0, 0.5] and u[2] == 0.5  # +y is the last row, -y the first, +x the middle column


def test_depth_one_frame_under_an_environment(oracle):
    """orct_trace_samples at depth 1: a miss is the environment colour of the sample's camera ray (the oracle's sampler and Camera.ray,
    the numpy rule), a hit is black (Shirley's scene has no emitter)"""
    w, h, spp = 48, 24, 2
    d = oracle.desc_shirley(w, h)
    env = S.random_environment(32, 16, 9)
    R = S.rotation([0.3, 1.0, 0.2], 120.0)
    xs, ys, ps = S.all_samples(w, h, spp)
    got = S.Restatement(d.ptr, d).trace_samples(env, T.BILINEAR, R, w, h, spp, 1, xs, ys, ps)
    o, dirs = S.camera_rays(oracle, d.d, w, h, spp, 1, xs, ys, ps)
    _, prim, _ = oracle.Scene(d.ptr, d).intersect_rays(o, dirs)
    miss = prim < 0
    assert 0.1 < miss.mean() < 0.9
    want = np.where(miss[:, None], T.environment_eval(env, T.BILINEAR, R, dirs), 0.0)
    assert np.array_equal(S.bits(got), S.bits(want + 0.0))  # (fma(1, c, 0) = c; a hit's fma(attn, 0, 0) = +0)


# ---------------------------------------------------------------------------------------------- the size limit (PTX_IMAGE_MAX_SIZE)
@pytest.mark.parametrize("W,H", T.LIMIT_SIZES)
def test_c_restatement_equals_numpy_at_the_size_limit(W, H):
    """products up to 2^62 on axes of up to 16384 texels: long long arithmetic in C against int64 in numpy"""
    img, u, v = T.limit_case(W, H)
    for bilinear in (0, T.BILINEAR):
        for wrap in WRAPS:
            got = S.c_image_eval(img, bilinear | wrap, u, v)
            assert np.array_equal(S.bits(got), S.bits(T.image_eval(img, bilinear | wrap, u, v))), (bilinear, wrap)


def test_the_size_limit_coordinates_tell_repeat_from_clamp_and_a_wrong_modulus():
    """what the case can see: beyond 2^32 a repeat axis lands on many texels (a clamp axis on the two edge ones), and an index reduced
    modulo 2^32 first (a 32-bit wrap) lands elsewhere for an n that does not divide 2^32"""
    W, H = 12289, 1
    img, u, v = T.limit_case(W, H)
    p = u * np.float64(W)
    far = (np.abs(p) >= 2.0 ** 32) & (np.abs(p) < 2.0 ** 62)
    ix = T._wrap(np.trunc(p[far]).astype(np.int64), W, True)
    assert len(np.unique(ix)) > 100
    narrow = T._wrap(np.trunc(p[far]).astype(np.int64) & 0xFFFFFFFF, W, True)
    assert (narrow != ix).sum() > 100


# ------------------------------------------------------------------------------------------------ whole paths with an image table
PW, PH, PSPP, PDEPTH = S.PATH_W, S.PATH_H, S.PATH_SPP, S.PATH_DEPTH


def plain_desc(name, oracle):
    return {"shirley": lambda: oracle.desc_shirley(PW, PH), "cornell": lambda: oracle.desc_cornell(PW, PH),
            "mesh": lambda: oracle.desc_ganesha_like(PW, PH, n_target=6000)}[name]()


@pytest.mark.parametrize("name", ["shirley", "cornell", "mesh"])
def test_no_image_and_no_environment_is_the_oracle(oracle, name):
    d = plain_desc(name, oracle)
    xs, ys, ps = S.all_samples(PW, PH, PSPP)
    o = oracle.Scene(d.ptr, d)
    want, _ = o.trace_samples(PW, PH, PSPP, PDEPTH, xs, ys, ps)
    o.close()
    ref = S.Restatement(d.ptr, d)
    assert np.array_equal(S.bits(ref.trace_samples_images(None, PW, PH, PSPP, PDEPTH, xs, ys, ps)), S.bits(want))
    # a table without an image is no table
    none = {0: (np.zeros((0, 0, 3)), 0)}
    assert np.array_equal(S.bits(ref.trace_samples_images(none, PW, PH, PSPP, PDEPTH, xs, ys, ps)), S.bits(want))
    ref.close()


@pytest.mark.parametrize("name", ["shirley", "cornell", "mesh"])
def test_the_even_checker_image_is_the_checker_along_whole_paths(oracle, name):
    import ctypes as C
    d, keep, index, (cw, ch), w, h = S.equivalence_case(name, oracle)
    ptr = C.pointer(d)
    xs, ys, ps = S.all_samples(w, h, PSPP)
    o = oracle.Scene(ptr, keep)
    want, _ = o.trace_samples(w, h, PSPP, PDEPTH, xs, ys, ps)
    o.close()
    even, odd = S.checker_colours(d, index)
    images = {index: (T.checker_image(cw, ch, even, odd), T.REPEAT_U | T.REPEAT_V)}
    ref = S.Restatement(ptr, keep)
    got = ref.trace_samples_images(images, w, h, PSPP, PDEPTH, xs, ys, ps)
    ref.close()
    assert np.array_equal(S.bits(got), S.bits(want))


@pytest.mark.parametrize("name", ["shirley", "mesh"])
def test_an_environment_alone_is_the_environment_tracer(oracle, name):
    d = plain_desc(name, oracle)
    env, R = S.random_environment(32, 16, 21), S.rotation([0.0, 1.0, 0.0], 75.0)
    xs, ys, ps = S.all_samples(PW, PH, PSPP)
    ref = S.Restatement(d.ptr, d)
    for flags in (0, T.BILINEAR):
        want = ref.trace_samples(env, flags, R, PW, PH, PSPP, PDEPTH, xs, ys, ps)
        got = ref.trace_samples_images(None, PW, PH, PSPP, PDEPTH, xs, ys, ps, env=env, env_flags=flags, R=R)
        assert np.array_equal(S.bits(got), S.bits(want)), flags
    ref.close()


def test_first_hit_albedo_is_the_numpy_rule_on_the_hits_own_coordinates(oracle):
    """cornell's image set: bilinear on the floor (4) and the metal sphere (6), nearest on the ceiling (5) and a wall (3); a
    dielectric shows (1, 1, 1), a miss the background, an entry without an image its texture"""
    case = S.path_case("cornell", oracle)
    d, images = case["desc"], case["images"]
    xs, ys, ps = S.all_samples(PW, PH, PSPP)
    ref = S.Restatement(d.ptr, d)
    albedo, hit, tex, uv = ref.first_hits(images, PW, PH, PSPP, PDEPTH, xs, ys, ps)
    plain, hit0, tex0, _ = ref.first_hits(None, PW, PH, PSPP, PDEPTH, xs, ys, ps)
    ref.close()
    assert np.array_equal(hit, hit0) and np.array_equal(tex, tex0)
    filters = set()
    for index, (img, flags) in images.items():
        on = tex == index
        assert on.sum() >= 32
        filters.add(flags & T.BILINEAR)
        assert np.array_equal(S.bits(albedo[on]), S.bits(T.image_eval(img, flags, uv[on, 0], uv[on, 1]))), index
    assert filters == {0, T.BILINEAR}
    rest = ~np.isin(tex, list(images))
    assert np.array_equal(S.bits(albedo[rest]), S.bits(plain[rest]))
    glass = (hit == 1) & (tex < 0)
    assert glass.sum() > 0 and (albedo[glass] == 1.0).all()
    assert (hit == 0).sum() > 0 and (albedo[hit == 0] == 0.0).all()  # cornell's background is black


# The conditions under which the GPU tests of whole paths mean something: on every scene and image set they use, each way of
# getting the lookup wrong changes the frame, and every imaged entry is seen directly.
SENSITIVITY_CASES = [("shirley", False), ("shirley", True), ("shirley_array", False), ("cornell", False), ("mesh", True)]


@pytest.mark.parametrize("name,with_env", SENSITIVITY_CASES)
def test_every_mistake_changes_the_frame(oracle, name, with_env):
    case = S.path_case(name, oracle)
    d, images = case["desc"], case["images"]
    env = dict(zip(("env", "env_flags", "R"), case["env"])) if with_env else {}
    xs, ys, ps = S.all_samples(PW, PH, PSPP)
    assert len(xs) == 8192
    ref = S.Restatement(d.ptr, d)
    want = ref.trace_samples_images(images, PW, PH, PSPP, PDEPTH, xs, ys, ps, **env)
    _, _, tex, uv = ref.first_hits(images, PW, PH, PSPP, PDEPTH, xs, ys, ps, **env)
    for index in images:
        assert (tex == index).sum() >= 32, (index, int((tex == index).sum()))
    if name.startswith("shirley"):  # a sphere's atan2 seam, where u reaches 0 and 1, is seen directly on an imaged entry
        assert any(uv[tex == i, 0].min() < 0.01 and uv[tex == i, 0].max() > 0.99 for i in images)

    def changed(got):
        return int((S.bits(got) != S.bits(want)).any(axis=1).sum())

    counts = {}
    for what, mutant in S.MUTANTS.items():
        counts[what] = changed(ref.trace_samples_images(images, PW, PH, PSPP, PDEPTH, xs, ys, ps, mutant=mutant, **env))
    counts["texture indices swapped"] = changed(ref.trace_samples_images(S.swapped(images, *case["swap"]), PW, PH, PSPP, PDEPTH, xs, ys,
                                                                         ps, **env))
    ref.close()
    print(name, "env" if with_env else "sky", counts)
    failed = {what: n for what, n in counts.items() if n < (8 if "toggled" in what else 64)}
    assert not failed, failed
