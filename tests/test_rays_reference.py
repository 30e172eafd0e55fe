"""tests/c/rays_oracle.c against the restatements it stands on, without a GPU: the path loop on explicit (ray, offset) pairs, fed
the cases' own camera rays and the offsets their samples have, must give what orcn_trace_samples (pinhole, lens) and
orcp_trace_samples (pose, pose + lens) give for those samples, bit for bit -- and one deliberately wrong variant (bounce dimensions
starting at 0 instead of 2) must not."""
import numpy as np
import pytest

import camera_pose_support as CS
import rays_support as RS
from rays_support import bits

W, H, SPP = RS.W, RS.H, RS.SPP


def _states(c):
    return {"pinhole": (None, False), "lens": (None, True), "pose": (c["poses"]["oblique"], False), "pose_lens": (c["poses"]["oblique"], True)}


@pytest.mark.parametrize("name", sorted(RS.CASES))
@pytest.mark.parametrize("state", ["pinhole", "lens", "pose", "pose_lens"])
def test_camera_rays_give_the_samples_radiance(oracle, name, state):
    c = RS.case(name, oracle)
    pose, lens = _states(c)[state]
    xs, ys, ps = RS.all_samples()
    offsets = RS.frame_offsets()
    for mode in RS.CASES[name]:
        for depth in RS.DEPTHS:
            rays = c["ref"].rays(pose, W, H, SPP, depth, xs, ys, ps, lens=c["lens"] if lens else None)
            want, want_seg = CS.restated(c, pose, depth, mode, lens=lens)
            got, seg = c["rays_ref"].trace_rays(rays, offsets, depth, RS.sampler_dim(depth, lens), c["images"], c["env"], mode, c["sampling"])
            assert (bits(got) == bits(want)).all(), (name, state, mode, depth)
            assert seg == want_seg


@pytest.mark.parametrize("name", sorted(RS.CASES))
def test_the_wrong_variant_differs(oracle, name):
    c = RS.case(name, oracle)
    xs, ys, ps = RS.all_samples()
    mode = RS.CASES[name][-1]
    rays = c["ref"].rays(None, W, H, SPP, 4, xs, ys, ps)
    right, _ = c["rays_ref"].trace_rays(rays, RS.frame_offsets(), 4, None, c["images"], c["env"], mode, c["sampling"])
    for label, mutant in RS.MUTANTS.items():
        wrong, _ = c["rays_ref"].trace_rays(rays, RS.frame_offsets(), 4, None, c["images"], c["env"], mode, c["sampling"], mutant=mutant)
        assert (bits(wrong) != bits(right)).any(), (name, label)


def test_null_offsets_are_the_ray_index_and_normalize_normalizes(oracle):
    c = RS.case("shirley", oracle)
    fam = RS.ray_families(c)
    n = len(fam["rays"])
    a, _ = c["rays_ref"].trace_rays(fam["rays"], None, 4)
    b, _ = c["rays_ref"].trace_rays(fam["rays"], np.arange(n), 4)
    assert (bits(a) == bits(b)).all()
    assert 200 <= n <= 320 and all(v > 0 for v in fam["families"].values()), fam["families"]
    lengths = np.linalg.norm(fam["scaled"][:, 3:], axis=1)
    assert lengths.min() < 1e-2 and lengths.max() > 1e2
    s, _ = c["rays_ref"].trace_rays(fam["scaled"], fam["offsets"], 4, normalize=True)
    u, _ = c["rays_ref"].trace_rays(fam["scaled"], fam["offsets"], 4, normalize=False)
    assert (bits(s) != bits(u)).any()  # the flag is not a no-op on these rays


def test_left_fold_is_a_left_fold():
    v = np.random.default_rng(3).random((12, 3))
    init = np.full((4, 3), 0.5)
    want = init.copy()
    for b in range(4):
        for k in range(3):
            want[b] = want[b] + v[3 * b + k]
    assert (bits(RS.left_fold(v, 3, init)) == bits(want)).all()
