"""The lat-long rule without a GPU: tests/projection_reference.py (numpy, from the header's text) against csrc/pt_projection.h compiled
for the host, bit for bit; and the property the rule exists for -- it is the inverse of the environment lookup.  For every sample of
a W x H panorama under the sampler's own jitter, texture_reference.environment_uv of the sample's direction lands in texel (x, y),
under the identity and under an oblique rotation with the environment's R set to the pose's transpose: zero mismatches, no tolerance.
"""
import numpy as np
import pytest

import camera_pose_support as CS
import projection_reference as PR
import texture_reference as TR
from lens_support import all_samples, bits

SIZES = [(1, 1), (8, 8), (9, 7), (13, 11), (33, 17), (64, 32)]
SPP, DEPTH = 3, 4
ROTATIONS = {"identity": np.eye(3), "oblique": CS.OBLIQUE_R}


def _edge_coordinates(rng):
    """film coordinates: random ones, the poles, the seam, the centre column, and values a hair inside the unit square"""
    e = np.array([0.0, 2.0 ** -53, 2.0 ** -30, 0.25, 0.5 - 2.0 ** -54, 0.5, 0.5 + 2.0 ** -53, 0.75, 1.0 - 2.0 ** -53, 1.0])
    grid = np.stack(np.meshgrid(e, e, indexing="ij"), axis=-1).reshape(-1, 2)
    return np.concatenate([rng.random((4000, 2)), grid])


@pytest.mark.parametrize("rotation", sorted(ROTATIONS))
def test_the_numpy_rule_is_the_product_header(oracle, rotation):
    R = ROTATIONS[rotation]
    o = np.array([0.3, -1.25, 7.0])
    cxcy = _edge_coordinates(np.random.default_rng(5))
    wo, wd = PR.latlong_rays(o, R, cxcy)
    go, gd = PR.product_latlong_rays(o, R, cxcy)
    assert np.array_equal(bits(go), bits(wo)) and (go == o).all()
    assert np.array_equal(bits(gd), bits(wd))
    assert np.abs(np.linalg.norm(wd, axis=1) - 1.0).max() < 1e-15


def test_the_directions_follow_the_environments_convention(oracle):
    """the centre column looks down +x, v = 0 (cy = 1, image row 0) is straight down as in the environment map, the seam is -x"""
    _, d = PR.latlong_rays(np.zeros(3), np.eye(3), [[0.5, 0.5], [0.5, 1.0], [0.5, 0.0], [0.0, 0.5], [0.75, 0.5], [0.25, 0.5]])
    want = np.array([[1.0, 0, 0], [0, -1.0, 0], [0, 1.0, 0], [-1.0, 0, 0], [0, 0, -1.0], [0, 0, 1.0]])
    assert np.abs(d - want).max() < 1e-15


@pytest.mark.parametrize("rotation", sorted(ROTATIONS))
@pytest.mark.parametrize("w, h", SIZES)
def test_the_environment_lookup_of_a_samples_direction_lands_in_its_texel(oracle, w, h, rotation):
    R = ROTATIONS[rotation]
    xs, ys, ps = all_samples(w, h, SPP)
    cxcy, jitter = PR.film_coordinates(w, h, SPP, 2 + 2 * DEPTH, xs, ys, ps)
    assert (jitter > 0.0).all() and (jitter < 1.0).all()  # no sample sits on a texel edge at these sizes
    _, d = PR.latlong_rays(np.array([1.0, 2.0, 3.0]), R, cxcy)
    u, v = TR.environment_uv(d, R.T)  # the environment's R takes scene space to the map's: the pose's transpose
    ix, iy = np.floor(u * w).astype(np.int64), np.floor(v * h).astype(np.int64)
    bad = (ix != xs) | (iy != ys)
    assert int(bad.sum()) == 0, f"{int(bad.sum())} of {len(xs)} samples leave their texel at {w} x {h} ({rotation})"
