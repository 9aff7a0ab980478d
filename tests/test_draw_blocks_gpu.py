"""The single-member proposal draw walks z in register blocks of 16 slots
(nb_kernels.hip, draw_product_single) and reads its slot table once per
workgroup.  Its proposals must be, bit for bit, those of the generic path
that a two-member union takes (draw_row, per-row slot tables): a union whose
two members are the same ellipsoid draws the same normals and the same radius
from the same Philox blocks whichever member a proposal picks, and the
single-member product promises the summation order of draw_row.  The
comparison held at every dimension below on the commit before the block walk
(whole z in registers) as well, so no recorded fixture stands in for it.
GPU only.

Shapes: every DT edge, the block edges at 16 and 32 slots, odd dimensions,
the benchmark's 50; 193 proposals = three full workgroups and one row."""

import numpy as np
import pytest
import torch

from helpers import upload

pytestmark = pytest.mark.gpu

DIMS = [2, 3, 16, 17, 31, 32, 33, 49, 50, 63, 64, 65, 96, 100, 127, 128]
N = 193
# (seed, offset): two seeds, one offset that is no multiple of 64
DRAWS = [(11, 0), (2**40 + 5, 0), (11, 1000003)]


def _ellipsoid(d, rng):
    from oracle import bounds_oracle as bo
    a = rng.normal(size=(d, d))
    cov = a @ a.T / d + np.eye(d)
    return bo.OEllipsoid.from_params(0.5 + 0.1 * rng.normal(size=d),
                                     np.linalg.cholesky(cov * 0.02))


def _mixture(n_ell, n_cube, rng):
    """Ellipsoid over n_ell dimensions, cube columns scattered between."""
    from oracle import bounds_oracle as bo
    dim_cube = np.zeros(n_ell + n_cube, bool)
    dim_cube[rng.choice(n_ell + n_cube, n_cube, replace=False)] = True
    return bo.OMixture.from_params(dim_cube, _ellipsoid(n_ell, rng))


def _single_and_twin(member):
    from oracle import bounds_oracle as bo
    one = bo.OUnion.from_members([member], unit=True)
    two = bo.OUnion.from_members([member, member], unit=True)
    b1, b2 = upload(one), upload(two)
    assert b1.n_members == 1 and b2.n_members == 2
    return one, b1, b2


def _assert_same_bits(b1, b2, n_dim):
    for seed, offset in DRAWS:
        x1 = b1.propose(seed, offset, N)
        x2 = b2.propose(seed, offset, N)
        assert x1.shape == (N, n_dim)
        assert bool(torch.isfinite(x1).all())
        assert torch.equal(x1, x2), (seed, offset, int((x1 != x2).sum()))


@pytest.mark.parametrize('d', DIMS)
def test_single_member_draw_is_the_generic_draw(d):
    _, b1, b2 = _single_and_twin(_ellipsoid(d, np.random.default_rng(d)))
    _assert_same_bits(b1, b2, d)


@pytest.mark.parametrize('n_ell,n_cube', [(5, 3), (40, 10)])
def test_single_member_mixture_draw_is_the_generic_draw(n_ell, n_cube):
    rng = np.random.default_rng(100 * n_ell + n_cube)
    _, b1, b2 = _single_and_twin(_mixture(n_ell, n_cube, rng))
    _assert_same_bits(b1, b2, n_ell + n_cube)


@pytest.mark.parametrize('d', [50, 100])
def test_single_member_draw_matches_oracle(d):
    """Guards against the two device paths being wrong together; tolerance of
    test_union_proposals_match_oracle."""
    from oracle import philox
    one, b1, _ = _single_and_twin(_ellipsoid(d, np.random.default_rng(d)))
    for seed, offset in DRAWS:
        x = b1.propose(seed, offset, N)
        x_o, _, _ = philox.union_propose(one, seed, offset, N)
        assert np.allclose(x.cpu().numpy(), x_o, rtol=0, atol=1e-12)


def test_single_member_mixture_draw_matches_oracle():
    """The staged slot table against the oracle's column placement."""
    from oracle import philox
    one, b1, _ = _single_and_twin(_mixture(40, 10, np.random.default_rng(7)))
    seed, offset = DRAWS[2]
    x = b1.propose(seed, offset, N)
    x_o, _, _ = philox.union_propose(one, seed, offset, N)
    assert np.allclose(x.cpu().numpy(), x_o, rtol=0, atol=1e-12)
