"""The camera-shutter rule (include/ptx.h, "camera shutter: motion blur between two poses") on the CPU.

* the product's own functions (csrc/pt_shutter.h compiled for the host), the numpy restatement (tests/shutter_reference.py) and the C
  one (tests/c/shutter_oracle.c) agree bit for bit: on a few thousand explicit (cx, cy, u, v, t) with times at both ends of [0, 1),
  angles from 0 to pi, axes along and off the coordinate axes and signed zeros, and through the sampler on every sample of a frame;
* T = 0, A = 0 gives the posed rule's ray (pt_camera_pose_ray / pt_latlong_ray) on the same inputs, compared as 0.0 + x;
* the ray at time t is the posed ray of the pose (o + t T, Rot(k, t A) R), that pose built from the closed-form rotation matrix:
  1e-12 absolute on origins of O(1) and on unit directions (the rule is about 40 roundings of 1.1e-16 on O(1) quantities);
* with a lens every sample's ray passes within 1e-12 F of the time-t camera's focus point;
* camera_shutter_between followed by the rule at t = 1 gives pose 1's ray within the same bar, for turns up to pi - 0.01 and none.
"""
import itertools

import numpy as np
import pytest

import camera_pose_reference as CR
import projection_reference as PR
import shutter_reference as SR
import shutter_support as S

bits = S.bits
CAM4 = (-0.3527, -0.1763, 0.7054, 0.3527)  # a 20-degree frustum at aspect 2
ORIGIN = (0.4, -1.3, 2.2)
ROT = S.rotation((0.3, 1.0, 2.0), 0.15)
LENS = (0.07, 9.0)
BAR = 1e-12
S3 = 1.0 / np.sqrt(3.0)
TIMES = (0.0, 5e-324, 2.0 ** -1022, 0.5, 1.0 - 2.0 ** -53)
ANGLES = (0.0, 1e-300, -1e-300, 1e-8, 0.1, -0.1, np.pi, -np.pi)
AXES = ((1.0, 0.0, 0.0), (0.0, -1.0, 0.0), (-0.0, 0.0, 1.0), (0.0, -0.0, -1.0), (S3, S3, S3), tuple(S.AXIS), (0.6, -0.0, -0.8))
TRANSLATIONS = ((0.0, 0.0, 0.0), (-0.0, 0.0, -0.0), (0.25, -0.5, 0.125), (1e-300, -3.0, 1e3))


def _inputs(n, seed):
    """(cxcy, uv): film coordinates over the frame with its corners and centre, lens pairs with u = 0 (the lens's centre) and v = 0"""
    rng = np.random.default_rng(seed)
    cxcy = rng.random((n, 2))
    cxcy[:5] = [(0.0, 0.0), (1.0, 1.0), (0.5, 0.5), (0.0, 1.0), (1.0, 0.0)]
    uv = rng.random((n, 2))
    uv[:3] = [(0.0, 0.0), (0.0, 0.75), (1.0 - 2.0 ** -53, 0.0)]
    return cxcy, uv


@pytest.mark.parametrize("kind", list(S.KINDS))
def test_the_product_is_the_numpy_restatement_bitwise(oracle, kind):
    """8 angles x 7 axes x 4 translations x 5 times x 9 samples = 10080 rays a kind, none of them NaN"""
    cxcy, uv = _inputs(9, 3)
    lens = LENS if kind == "lens" else None
    n = 0
    for A, k, T in itertools.product(ANGLES, AXES, TRANSLATIONS):
        t = np.repeat(TIMES, len(cxcy))
        cc, uu = np.tile(cxcy, (len(TIMES), 1)), np.tile(uv, (len(TIMES), 1))
        got = S.product_rays(kind, CAM4, ORIGIN, ROT, T, k, A, cc, t, lens, uu)
        o, d = SR.shutter_rays(CAM4, ORIGIN, ROT, T, k, A, cc, t, lens, uu if lens else None, latlong=(kind == "latlong"))
        want = np.concatenate([o, d], axis=1)
        assert np.isfinite(want).all()
        assert np.array_equal(bits(got), bits(want)), (A, k, T)
        n += len(t)
    assert n == 10080


@pytest.mark.parametrize("state", ["both", "turn", "move", "pose_off", "lens", "latlong"])
def test_the_restatements_agree_through_the_sampler(oracle, state):
    """every sample of the frame: the C restatement reads its own sampler (d dimensions, the time last, the lens pair before it), the
    numpy one the oracle's"""
    c = S.case("shirley", oracle)
    st = c["states"][state]
    xs, ys, ps = S.all_samples()
    for depth in (0, 4):
        by_c = c["sref"].rays(c, st, S.W, S.H, S.SPP, depth, xs, ys, ps)
        by_numpy = S.numpy_rays(oracle, c, st, S.W, S.H, S.SPP, depth, xs, ys, ps)
        assert np.array_equal(bits(by_c), bits(by_numpy)), depth
    # the shutter is not ignored: against the same state without it (another table: every sample's direction differs)
    pose = st.pose or S.Pose(S.ZERO, S.IDENTITY)
    if not st.latlong:
        still = c["ref"].rays(pose, S.W, S.H, S.SPP, 4, xs, ys, ps, c["lens"] if st.lens else None)
        assert (bits(still[:, 3:]) != bits(by_c[:, 3:])).any(axis=1).all()
    if state != "turn":  # the origin moves with the sample's time: one origin per sampler offset
        offsets = ys.astype(np.int64) * S.W + xs + ps.astype(np.int64) * S.SPP
        assert len(np.unique(by_c[:, 0])) == len(np.unique(offsets)) > len(xs) // 4


@pytest.mark.parametrize("kind", list(S.KINDS))
@pytest.mark.parametrize("k", [(0.0, 0.0, 0.0), (1.0, 0.0, 0.0), tuple(S.AXIS)])
def test_no_motion_is_the_posed_ray(oracle, kind, k):
    """T = 0, A = 0: S(w) = w and ot = o, so the rule gives the posed ray of the same (cx, cy, u, v) up to the sign of a zero -- compared
    as 0.0 + x -- at any time"""
    cxcy, uv = _inputs(600, 5)
    lens = LENS if kind == "lens" else None
    t = np.tile(TIMES, len(cxcy) // len(TIMES))
    for o, R in ((ORIGIN, ROT), (S.ZERO, S.IDENTITY)):
        moving = S.product_rays(kind, CAM4, o, R, S.ZERO, k, 0.0, cxcy, t, lens, uv)
        still = S.product_rays(kind, CAM4, o, R, S.ZERO, k, 0.0, cxcy, t, lens, uv, shutter=False)
        assert np.array_equal(bits(0.0 + moving), bits(0.0 + still))
        # and the restatements of the posed rules
        if kind == "latlong":
            want = np.concatenate(PR.latlong_rays(o, R, cxcy), axis=1)
        else:
            want = np.concatenate(CR.pose_rays(CAM4, o, R, cxcy, lens, uv if lens else None), axis=1)
        assert np.array_equal(bits(0.0 + moving), bits(0.0 + want))


def _pose_at(T, k, A, t):
    """(o + t T, Rot(k, t A) R) in closed form"""
    return np.asarray(ORIGIN) + t * np.asarray(T), SR.rotation_matrix(k, t * A) @ ROT


@pytest.mark.parametrize("kind", list(S.KINDS))
def test_the_ray_at_time_t_is_the_posed_ray_of_the_pose_at_time_t(oracle, kind):
    cxcy, uv = _inputs(64, 7)
    lens = LENS if kind == "lens" else None
    worst = 0.0
    for A, k, T, t in itertools.product((0.0, 1e-8, 0.1, -2.5, np.pi), AXES, TRANSLATIONS[2:3] + ((0.0, 0.0, 0.0),), TIMES[1:]):
        got = S.product_rays(kind, CAM4, ORIGIN, ROT, T, k, A, cxcy, t, lens, uv)
        o, R = _pose_at(T, k, A, t)
        if kind == "latlong":
            want = np.concatenate(PR.latlong_rays(o, R, cxcy), axis=1)
        else:
            want = np.concatenate(CR.pose_rays(CAM4, o, R, cxcy, lens, uv if lens else None), axis=1)
        worst = max(worst, float(np.abs(got - want).max()))
    print(f"{kind}: largest difference from the posed ray of the pose at time t: {worst:.3e}")
    assert worst <= BAR


def test_with_a_lens_every_ray_passes_through_the_focus_point_of_the_camera_at_time_t(oracle):
    cxcy, uv = _inputs(64, 11)
    radius, F = LENS
    worst = 0.0
    for A, k, t in itertools.product((0.0, 0.1, -2.5, np.pi), AXES, TIMES):
        T = TRANSLATIONS[2]
        rays = S.product_rays("lens", CAM4, ORIGIN, ROT, T, k, A, cxcy, t, LENS, uv)
        o, R = _pose_at(T, k, A, t)
        q = np.stack([CAM4[0] + CAM4[2] * cxcy[:, 0], CAM4[1] + CAM4[3] * cxcy[:, 1], np.full(len(cxcy), -1.0)], axis=1)
        focus = o + (F * q) @ R.T
        to = focus - rays[:, :3]
        off = to - (to * rays[:, 3:]).sum(axis=1, keepdims=True) * rays[:, 3:]  # the part of (focus - origin) across the ray
        worst = max(worst, float(np.linalg.norm(off, axis=1).max()))
        assert (np.linalg.norm(rays[:, :3] - o, axis=1) <= radius * (1.0 + 1e-12)).all()  # and starts on the lens
    print(f"largest distance from a ray to its focus point: {worst:.3e} (F = {F})")
    assert worst <= BAR * F


@pytest.mark.parametrize("angle", [0.0, 1e-9, 0.3, -1.2, 2.0, np.pi - 0.01, -(np.pi - 0.01)])
@pytest.mark.parametrize("axis", [(0.0, 1.0, 0.0), tuple(S.AXIS), (0.6, 0.0, -0.8)])
def test_shutter_between_two_poses_ends_at_the_second(oracle, angle, axis):
    import path_tracer_ocaml_amd as P
    o1 = np.asarray(ORIGIN) + np.array([0.5, -0.25, 0.75])
    R1 = SR.rotation_matrix(axis, angle) @ ROT
    T, k, A = P.camera_shutter_between(ORIGIN, ROT, o1, R1)
    assert np.array_equal(T, o1 - np.asarray(ORIGIN)) and 0.0 <= A <= np.pi
    if angle == 0.0:
        assert A == 0.0 and (k == 0.0).all()  # no turn: the setter takes a zero axis with angle 0
    else:
        assert abs(np.linalg.norm(k) - 1.0) <= 1e-9 and abs(A - abs(angle)) <= 1e-9  # what the setter asks of them
        assert np.abs(k * np.sign(angle) - np.asarray(axis)).max() <= 1e-6 or abs(angle) < 1e-6
    cxcy, uv = _inputs(64, 13)
    for kind, lens in (("pose", None), ("lens", LENS), ("latlong", None)):
        got = S.product_rays(kind, CAM4, ORIGIN, ROT, T, k, A, cxcy, 1.0, lens, uv)
        if kind == "latlong":
            want = np.concatenate(PR.latlong_rays(o1, R1, cxcy), axis=1)
        else:
            want = np.concatenate(CR.pose_rays(CAM4, o1, R1, cxcy, lens, uv if lens else None), axis=1)
        assert float(np.abs(got - want).max()) <= BAR, kind
