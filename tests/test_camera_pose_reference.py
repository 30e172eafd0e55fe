"""The camera-pose rule (include/ptx.h, "camera pose: a movable camera, no rebuild") on the CPU: the C restatement
(tests/c/camera_pose_oracle.c), the numpy one (tests/camera_pose_reference.py) and the product's own function
(csrc/pt_camera_pose.h compiled for the host) agree bit for bit on every sample of two frames; the identity pose at origin 0 is the
pinhole's ray and, with a lens, the lens's, bit for bit; pth_camera_pose_look_at points the posed camera at its target and poses the
scene's own camera home within rounding; and a scene built for camera A and posed to camera B renders what the scene built for B
renders, except where rounding pushes a sample across a silhouette.
"""
import numpy as np
import pytest

import camera_pose_reference as CR
import camera_pose_support as S
from path_tracer_ocaml_amd import host

bits = S.bits
FRAMES = ((13, 7, 4), (64, 40, 2))
DEPTH = 4
SKEW = S.rotation((-0.3, 0.8, 0.5), 2.1)
POSES = {"oblique": ((0.4, -1.3, 2.2), S.OBLIQUE_R), "skew": ((-7.5, 0.0, 1e-3), SKEW), "identity": ((0.0, 0.0, 0.0), np.eye(3))}
LENS = (0.07, 9.0)


def _film(oracle, width, height, spp, dim):
    """every sample of the frame: offsets, film coordinates and the sampler's last two dimensions, from the header's text alone"""
    xs, ys, ps = S.all_samples(width, height, spp)
    off = (ys * width) + xs + (ps * spp)
    get = lambda k: oracle.lds_get_vec(dim, off, np.full(len(off), k))  # noqa: E731
    cx = (xs.astype(np.float64) + get(0)) * (1.0 / width)
    cy = 1.0 - ((ys.astype(np.float64) + get(1)) * (1.0 / height))
    return (xs, ys, ps), np.stack([cx, cy], axis=1), np.stack([get(dim - 2), get(dim - 1)], axis=1)


@pytest.fixture(scope="module")
def shirley(oracle):
    return {(w, h): S.case("shirley", oracle, w, h) for w, h, _ in FRAMES}


@pytest.mark.parametrize("width, height, spp", FRAMES)
@pytest.mark.parametrize("lens", [None, LENS])
@pytest.mark.parametrize("override", [False, True])
@pytest.mark.parametrize("pose", list(POSES))
def test_the_restatements_and_the_product_agree_bitwise(oracle, shirley, width, height, spp, lens, override, pose):
    c = shirley[(width, height)]
    o, R = POSES[pose]
    assert pose == "identity" or ((np.asarray(R) < 0).any() and (np.asarray(R) > 0).any())  # mixed signs
    own = S.cam4_of(c["desc"])
    view = (0.8 * own[0], 1.1 * own[1], 1.7 * own[2], 2.0 * own[3]) if override else None
    dim = (4 if lens else 2) + 2 * DEPTH
    (xs, ys, ps), cxcy, uv = _film(oracle, width, height, spp, dim)
    # through the sampler: the C restatement's own offsets, alphas and film coordinates
    sampled = c["ref"].rays(S.Pose(o, R, view), width, height, spp, DEPTH, xs, ys, ps, lens)
    # on the film coordinates restated here
    cam4 = view or own
    by_c = S.c_pose_rays(cam4, o, R, cxcy, lens, uv)
    by_numpy = np.concatenate(CR.pose_rays(cam4, o, R, cxcy, lens, uv), axis=1)
    by_product = S.product_pose_rays(cam4, o, R, cxcy, lens, uv)
    assert np.array_equal(bits(sampled), bits(by_c))
    assert np.array_equal(bits(by_numpy), bits(by_c))
    assert np.array_equal(bits(by_product), bits(by_c))
    if pose != "identity":  # and the pose is not ignored
        home = c["ref"].rays(None, width, height, spp, DEPTH, xs, ys, ps, lens)
        assert (bits(sampled) != bits(home)).any(axis=1).all()


@pytest.mark.parametrize("width, height, spp", FRAMES)
@pytest.mark.parametrize("lens", [None, LENS])
def test_the_identity_pose_is_the_scenes_own_ray(oracle, shirley, width, height, spp, lens):
    """bit for bit on every sample: the pinhole's ray, and with a lens on the lens's (the restatements of the existing rules).  The
    one caveat the header states, the sign of a zero, does not arise on these samples."""
    c = shirley[(width, height)]
    xs, ys, ps = S.all_samples(width, height, spp)
    home = c["ref"].rays(None, width, height, spp, DEPTH, xs, ys, ps, lens)
    posed = c["ref"].rays(S.Pose(S.ZERO, S.IDENTITY), width, height, spp, DEPTH, xs, ys, ps, lens)
    assert np.array_equal(bits(posed), bits(home))
    if lens is None:
        assert (home[:, :3] == 0.0).all()
    # the product's function too
    dim = (4 if lens else 2) + 2 * DEPTH
    _, cxcy, uv = _film(oracle, width, height, spp, dim)
    assert np.array_equal(bits(S.product_pose_rays(S.cam4_of(c["desc"]), S.ZERO, S.IDENTITY, cxcy, lens, uv)), bits(home))
    # and whole paths
    a, _ = c["ref"].trace_samples(None, width, height, spp, DEPTH, xs, ys, ps, lens=lens)
    b, _ = c["ref"].trace_samples(S.Pose(S.ZERO, S.IDENTITY), width, height, spp, DEPTH, xs, ys, ps, lens=lens)
    assert np.array_equal(bits(a), bits(b)) and float(a.max()) > 0.0


# ------------------------------------------------------------------------------------------------ pth_camera_pose_look_at
SHIRLEY_EYE, SHIRLEY_TARGET, UP = (13.0, 2.0, 4.5), (0.0, 0.0, 0.0), (0.0, 1.0, 0.0)
CAMERA_B = ((9.0, 3.5, -6.0), (0.5, 0.4, 0.3), 28.0)  # eye, target, fov
# A camera with the orientation of Shirley's own, moved (eye and target by the same vector) and with another field of view.  The
# background, the normals and the texture coordinates stay in the scene's space (include/ptx.h), so a scene REBUILT for a camera that
# is turned against the first has another sky gradient and another checker phase in every pixel: only a camera that keeps the
# orientation makes "posed" and "rebuilt" the same picture.
MOVE = (-3.0, 1.5, 2.0)
CAMERA_B_MOVED = (tuple(e + m for e, m in zip(SHIRLEY_EYE, MOVE)), tuple(e + m for e, m in zip(SHIRLEY_TARGET, MOVE)), 31.0)


def test_host_scenes_record_their_camera():
    hs = host.shirley_spheres(16, 8)
    cam = hs.camera
    assert tuple(cam["eye"]) == SHIRLEY_EYE and tuple(cam["target"]) == SHIRLEY_TARGET and cam["fov_deg"] == 20.0
    view, m = host.camera_create(SHIRLEY_EYE, SHIRLEY_TARGET, UP, 2.0, 20.0)
    assert np.array_equal(bits(m), bits(cam["look_at"]))
    d = hs.d.camera
    assert view == (d.lower_left_x, d.lower_left_y, d.view_x, d.view_y)


@pytest.mark.parametrize("eye, target, fov", [CAMERA_B, ((-4.0, 0.7, 11.0), (1.0, 1.0, -2.0), 55.0), ((0.0, 30.0, 0.1), (0.0, 0.0, 0.0), 10.0)])
def test_look_at_points_the_film_centre_at_the_target(eye, target, fov):
    _, scene_m = host.camera_create(SHIRLEY_EYE, SHIRLEY_TARGET, UP, 2.0, 20.0)
    o, R, view = host.camera_pose_look_at(scene_m, eye, target, UP, 1.5, fov)
    _, d = CR.pose_rays(view, o, R, [(0.5, 0.5)])
    # the target in the scene's space: Mat4.transform scene_look_at target
    t = scene_m[:3, :3] @ np.asarray(target) + scene_m[:3, 3]
    want = (t - o) / np.linalg.norm(t - o)
    assert 1.0 - float(d[0] @ want) <= 1e-12
    assert np.abs(R @ R.T - np.eye(3)).max() <= 1e-9 and np.linalg.det(R) > 0.0  # what the setter asks of it
    assert view == host.camera_create(eye, target, UP, 1.5, fov)[0]


def test_look_at_home_is_the_identity_within_rounding():
    """eye and target equal to the scene's own: the identity within 1e-15 and the origin within 1e-12 of the scene's units -- NOT
    exactly (dot products of unit vectors round), which is why "off" and "posed back home" are different states"""
    for build, aspect in ((host.shirley_spheres, 2.0), (host.cornell_box, 1.0)):
        cam = build(16, int(16 / aspect)).camera
        o, R, _ = host.camera_pose_look_at(cam["look_at"], cam["eye"], cam["target"], cam["up"], aspect, cam["fov_deg"])
        assert np.abs(R - np.eye(3)).max() <= 1e-15
        assert np.abs(o).max() <= 1e-12


def _shirley_pair(oracle, width, height):
    """(Shirley built for camera A -- its own -- with the pose of camera B, Shirley's geometry built for camera B): the second is the
    first's spheres moved from A's space to B's by the exact same Mat4.transform the host builder applies"""
    import ctypes as C
    from path_tracer_ocaml_amd import abi
    hs = host.shirley_spheres(width, height)
    cam = hs.camera
    eye, target, fov = CAMERA_B_MOVED
    aspect = width / height
    pose = S.Pose(*host.camera_pose_look_at(cam["look_at"], eye, target, UP, aspect, fov))
    view_b, m_b = host.camera_create(eye, target, UP, aspect, fov)
    # world positions: undo A's look_at (a rigid motion: its inverse is R^T (p - t)), then apply B's as the builder does
    d = hs.d
    n = d.n_spheres
    pa = np.stack([np.ctypeslib.as_array(p, shape=(n,)) for p in (d.sphere_x, d.sphere_y, d.sphere_z)], axis=1)
    ma = cam["look_at"]
    rel = pa - ma[:3, 3]  # (sums written out: no BLAS, the same bits on every machine)
    world = np.stack([((rel[:, 0] * ma[0, j]) + (rel[:, 1] * ma[1, j])) + (rel[:, 2] * ma[2, j]) for j in range(3)], axis=1)
    pb = np.stack([(((world[:, 0] * m_b[i, 0]) + (world[:, 1] * m_b[i, 1])) + (world[:, 2] * m_b[i, 2])) + (1.0 * m_b[i, 3]) for i in range(3)], axis=1)
    xb, yb, zb = (np.ascontiguousarray(pb[:, i]) for i in range(3))
    db = abi.SceneDesc()
    C.memmove(C.byref(db), C.byref(d), C.sizeof(abi.SceneDesc))
    db.sphere_x, db.sphere_y, db.sphere_z = (a.ctypes.data_as(abi.c_double_p) for a in (xb, yb, zb))
    db.camera = abi.Camera(*view_b)
    keep = (hs, xb, yb, zb, db)
    return S.Restatement(hs.ptr, hs), pose, S.Restatement(C.pointer(db), keep)


MEASURED_SHARE = 0.0  # of 4608 pixels, on the restatement (the largest relative difference of any pixel's sums: 3.44e-11)


def test_a_posed_scene_is_the_scene_rebuilt_for_that_camera(oracle):
    """Shirley 96 x 48, spp 4, depth 4, built for camera B (CAMERA_B_MOVED) against the same scene built for its own camera and posed
    to B.  The sampler offsets are identical, so only samples that rounding pushes across a silhouette, a checker edge or a Fresnel
    branch differ.  Measured on the restatement: 0 of 4608 pixels (0 %) have raw sums that differ by more than 1e-9 relative; the
    largest relative difference of any pixel is 3.44e-11.  The cap is four times the measured share, which is 0 -- under 2 %."""
    w, h, spp, depth = 96, 48, 4, 4
    posed_scene, pose, rebuilt_scene = _shirley_pair(oracle, w, h)
    xs, ys, ps = S.all_samples(w, h, spp)
    a, _ = posed_scene.trace_samples(pose, w, h, spp, depth, xs, ys, ps)
    b, _ = rebuilt_scene.trace_samples(None, w, h, spp, depth, xs, ys, ps)
    sa, sb = S.pass_order_sums(a, w, h, spp), S.pass_order_sums(b, w, h, spp)

    def differing(x):
        return np.abs(x - sb).max(axis=2) / np.maximum(np.abs(sb).max(axis=2), 1e-300) > 1e-9
    share = float(differing(sa).mean())
    print(f"pixels whose raw sums differ by more than 1e-9 relative: {share * 100:.4f} % ({int(differing(sa).sum())} of {w * h})")
    cap = 4.0 * MEASURED_SHARE
    assert cap < 0.02
    assert share <= cap
    assert float(sb.max()) > 0.5 and not np.array_equal(bits(sa), bits(sb))  # the same picture, not the same arithmetic
    # the pose matters: the scene without it is another picture in most pixels
    c, _ = posed_scene.trace_samples(None, w, h, spp, depth, xs, ys, ps)
    assert differing(S.pass_order_sums(c, w, h, spp)).mean() > 0.5
