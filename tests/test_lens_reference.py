"""The thin-lens rule (include/ptx.h, "thin-lens camera: aperture and focus distance") on the CPU: the C restatement
(tests/c/lens_oracle.c), the numpy one (tests/lens_reference.py) and the product's own function (csrc/pt_lens.h compiled for the host)
agree bit for bit, the rule has the properties a lens must have within bounds derived from its rounding, each mutant of the
restatement fails one of these checks, and the inputs of the GPU tests tell a lens render from a pinhole render.

Rounding, with u = 2^-53 (every operation of the rule is one correctly rounded IEEE operation, except hypot, sin and cos of pt_math.h:
< 1 ulp, i.e. a relative error below 2u):
  d = s * e, s = 1 / hypot(..): hypot 2u, the division u, the product u -> every component of d is a common factor times the exact
  e_i, off by at most 4u; e_i = P_i - L_i carries u more.  The check's own arithmetic (s = P.z / d.z, L + s * d) adds a division, a
  product and a sum.  The point of a ray in the plane z = -F is therefore within 16 u (|P.x| + |P.y| + |L.x| + |L.y| + F) of P.
  |L| = A r hypot(cos, sin): r <= 1, cos and sin 2u each, three products -> |L| <= A (1 + 8u).
  |L|^2 / A^2 = u_lens (1 + at most 16u); a mean of 256 terms adds at most 8 more roundings -> |mean - 1/2| <= 32u.
"""
import numpy as np
import pytest

import lens_reference as LR
import lens_support as S

U = 2.0 ** -53
bits = S.bits
CAM = (-1.3, -0.8, 2.6, 1.6)  # (llx, lly, vx, vy): a 16:10 film


def _inputs(n=4096, seed=3):
    rng = np.random.default_rng(seed)
    edge = [0.0, 0.25, 0.5, 1.0 - 2.0 ** -53]
    uv = np.array([(a, b) for a in edge for b in edge] + rng.uniform(0.0, 1.0, (n - 16, 2)).tolist())
    return rng.uniform(0.0, 1.0, (n, 2)), uv


@pytest.mark.parametrize("lens", [(0.05, 10.0), (1.5, 0.75), (1e-9, 1e6)])
def test_the_restatements_and_the_product_agree_bitwise(oracle, lens):
    cxcy, uv = _inputs()
    c = S.c_lens_rays(CAM, *lens, cxcy, uv)
    L, d = LR.lens_rays(CAM, *lens, cxcy, uv)
    assert np.array_equal(bits(c[:, :3]), bits(L)) and np.array_equal(bits(c[:, 3:]), bits(d))
    assert np.array_equal(bits(S.product_lens_rays(CAM, *lens, cxcy, uv)), bits(c))


def _miss_of_focus_point(rays, P):
    L, d = rays[:, :3], rays[:, 3:]
    s = P[:, 2] / d[:, 2]  # L.z = 0: the parameter that reaches z = P.z = -F
    return np.abs(L + s[:, None] * d - P).max(axis=1)


def _focus_bound(rays, P, F):
    return 16.0 * U * (np.abs(P[:, 0]) + np.abs(P[:, 1]) + np.abs(rays[:, 0]) + np.abs(rays[:, 1]) + F)


@pytest.mark.parametrize("lens", [(0.05, 10.0), (1.5, 0.75)])
def test_every_ray_of_a_film_point_passes_through_its_focus_point(oracle, lens):
    A, F = lens
    _, uv = _inputs()
    for cxcy1 in ((0.5, 0.5), (0.03, 0.91), (1.0, 0.0)):
        cxcy = np.tile(cxcy1, (len(uv), 1))
        rays = S.c_lens_rays(CAM, A, F, cxcy, uv)
        P = LR.focus_points(CAM, F, cxcy)
        assert (P[:, 2] == -F).all()
        assert (_miss_of_focus_point(rays, P) <= _focus_bound(rays, P, F)).all(), cxcy1
        # the lens: z = 0 exactly, within the radius; directions are unit vectors looking down -z
        assert (bits(rays[:, 2]) == 0).all()
        assert (np.hypot(rays[:, 0], rays[:, 1]) <= A * (1.0 + 8.0 * U)).all()
        assert (np.abs(np.linalg.norm(rays[:, 3:], axis=1) - 1.0) <= 8.0 * U).all() and (rays[:, 5] < 0.0).all()
        assert np.unique(bits(rays[:, :2]), axis=0).shape[0] > len(uv) // 2  # the origins do spread


def _midpoints(n=16):
    m = (np.arange(n) + 0.5) / n
    return np.array([(a, b) for a in m for b in m])


def _disc_mean(rays, A):
    return float(np.mean((rays[:, 0] * rays[:, 0] + rays[:, 1] * rays[:, 1]) / (A * A)))


def test_the_lens_is_sampled_uniformly_by_area(oracle):
    uv = _midpoints()
    assert float(np.mean(uv[:, 0])) == 0.5  # exactly: the midpoints of 16 cells are dyadic
    for A, F in ((0.05, 10.0), (1.5, 0.75)):
        rays = S.c_lens_rays(CAM, A, F, np.full((len(uv), 2), 0.5), uv)
        assert abs(_disc_mean(rays, A) - 0.5) <= 32.0 * U


def test_each_mutant_fails_a_check(oracle):
    A, F = 0.05, 10.0
    _, uv = _inputs()
    cxcy = np.tile((0.03, 0.91), (len(uv), 1))
    P = LR.focus_points(CAM, F, cxcy)
    along = S.c_lens_rays(CAM, A, F, cxcy, uv, S.MUTANTS["focus measured along the ray"])
    assert not (_miss_of_focus_point(along, P) <= _focus_bound(along, P, F)).all()
    mid = _midpoints()
    linear = S.c_lens_rays(CAM, A, F, np.full((len(mid), 2), 0.5), mid, S.MUTANTS["r = u for sqrt u"])
    assert abs(_disc_mean(linear, A) - 0.5) > 32.0 * U
    # the lens pair's dimensions: the numpy restatement takes them from d - 2 and d - 1 of the sampler
    c = S.case("shirley", oracle)
    xs, ys, ps = S.all_samples()
    depth = 4
    good, cxcy = c["ref"].rays(c["lens"], S.W, S.H, S.SPP, depth, xs, ys, ps)
    dims23, _ = c["ref"].rays(c["lens"], S.W, S.H, S.SPP, depth, xs, ys, ps, S.MUTANTS["lens pair at dimensions 2 and 3"])
    want = _numpy_sample_rays(oracle, c, depth, xs, ys, ps)
    assert np.array_equal(bits(good), bits(want))
    assert (bits(dims23) != bits(want)).any(axis=1).all()


def _numpy_sample_rays(oracle, c, depth, xs, ys, ps, width=S.W, height=S.H, spp=S.SPP):
    """the samples' lens rays from the header's text alone: offsets, the d = 4 + 2 depth sampler, the film coordinates, the rule"""
    d = 4 + 2 * depth
    off = (ys * width) + xs + (ps * spp)
    get = lambda dim: oracle.lds_get_vec(d, off, np.full(len(off), dim))  # noqa: E731
    cx = (xs.astype(np.float64) + get(0)) * (1.0 / width)
    cy = 1.0 - ((ys.astype(np.float64) + get(1)) * (1.0 / height))
    cam = c["desc"].contents.camera
    cam4 = (cam.lower_left_x, cam.lower_left_y, cam.view_x, cam.view_y)
    L, dirs = LR.lens_rays(cam4, *c["lens"], np.stack([cx, cy], axis=1), np.stack([get(d - 2), get(d - 1)], axis=1))
    return np.concatenate([L, dirs], axis=1)


@pytest.mark.parametrize("name", list(S.CASES))
def test_lens_off_is_the_oracle(oracle, name):
    """radius 0 is not a lens of radius 0: the restated loop with the lens off is orc_trace_samples bit for bit (modes 0, no images,
    no environment: what the oracle itself states), and on every case's own state it is the existing restatements' loop"""
    c = S.case(name, oracle)
    xs, ys, ps = S.all_samples()
    for depth in S.DEPTHS:
        if name in ("shirley", "shirley_array", "cornell", "mesh"):
            got, _ = c["ref"].trace_samples((0.0, 1.0), S.W, S.H, S.SPP, depth, xs, ys, ps)
            assert np.array_equal(bits(got), bits(c["ref"].oracle_samples(S.W, S.H, S.SPP, depth, xs, ys, ps))), (name, depth)
    if name == "envlight":
        import envlight_support as ES
        img, flags, R = c["env"]
        want = ES.Restatement(c["desc"], c["keep"]).trace_samples(img, flags, R, 2, True, S.W, S.H, S.SPP, 4, xs, ys, ps)
        assert np.array_equal(bits(S.restated(c, 4, 2, lens=False)[0]), bits(want))
    if name == "image":
        import texture_support as TS
        want = TS.Restatement(c["desc"], c["keep"]).trace_samples_images(c["images"], S.W, S.H, S.SPP, 4, xs, ys, ps)
        assert np.array_equal(bits(S.restated(c, 4, 0, lens=False)[0]), bits(want))


@pytest.mark.parametrize("name", list(S.CASES))
def test_the_gpu_tests_inputs_tell_a_lens_from_a_pinhole(oracle, name):
    """so that a GPU that ignored the lens cannot pass tests/test_gpu_lens.py"""
    c = S.case(name, oracle)
    xs, ys, ps = S.all_samples()
    A, F = c["lens"]
    assert A > 0.0 and F > 0.0
    for depth in S.DEPTHS:
        lens_rays, _ = c["ref"].rays(c["lens"], S.W, S.H, S.SPP, depth, xs, ys, ps)
        pin_rays, _ = c["ref"].rays((0.0, 1.0), S.W, S.H, S.SPP, depth, xs, ys, ps)
        assert (bits(lens_rays) != bits(pin_rays)).any(axis=1).all(), (name, depth)
    for mode in S.CASES[name]:
        for depth in (1, 4):
            a, b = S.restated(c, depth, mode)[0], S.restated(c, depth, mode, lens=False)[0]
            assert (bits(a) != bits(b)).any(), (name, mode, depth)
            assert float(a.max()) > 0.0
