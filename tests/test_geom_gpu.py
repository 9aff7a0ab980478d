"""The geometric kernel (nb_geom.hip: r2 of a bound without emulators, overlap
count of the outer members) at every tile count it is compiled for, and the
exports without a work argument (nb_contains, nb_contains_any,
nb_first_containing, nb_accept), which run the two stages in stream-ordered
work space.  GPU only."""

import ctypes as C

import numpy as np
import pytest
import torch

from conftest import load_golden
from helpers import upload, near_boundary, nautilus_from_golden

pytestmark = pytest.mark.gpu

# both sides of every tile boundary (16 DT) and of the switch from two tiles
# per wavefront to one (64 | 65)
DIMS = [1, 16, 17, 33, 50, 64, 65, 81, 100, 113, 128]


@pytest.fixture(scope='module')
def dev():
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    from nautilus_amd import device
    return device


def _call(fn, handle, x, out, stream, *head):
    from nautilus_amd import _lib
    _lib.check(fn(handle, *head, C.c_void_p(x.data_ptr()), x.shape[0],
                  C.c_void_p(out.data_ptr()), C.c_void_p(stream.cuda_stream)))
    return out


def gaussian(d):
    """Mean and Cholesky factor of a random SPD covariance in d dimensions."""
    rng = np.random.default_rng(900 + d)
    a = rng.normal(size=(d, d))
    chol = np.linalg.cholesky(0.01 * (a @ a.T / d + np.eye(d)))
    return rng, 0.5 + 0.1 * rng.normal(size=d), chol


@pytest.mark.parametrize('d', DIMS)
def test_r2_every_tile_count(dev, d):
    """r2 mode: ``neural_score`` of an emulator-less bound against numpy's
    |L^-1 (x - mu)|^2, bit for bit against the pipelined kernel's r2 of the
    same ellipsoid (a bound with one dummy network: nb_eval_fast_kernel),
    column 1 zero, the counters -- for one row, ragged passes, several
    workgroups and, at d = 50, more 128-row passes than workgroups."""
    from scipy.linalg import solve_triangular
    from oracle import mlp_oracle as mo
    rng, mean, chol = gaussian(d)
    ell = dev.member(mean, chol)
    plain = dev.DeviceBound(d, [], None, False, [dict(ellipsoid=ell)])
    with_net = dev.DeviceBound(d, [], None, False, [dict(
        ellipsoid=ell, score_predict_min=0.0,
        mlp=dict(mean=np.zeros(d), scale=np.ones(d),
                 nets=[mo.glorot_init(d, 0)[:2]]))])
    assert plain.n_networks == 0 and with_net.n_networks == 1
    n_max = 33000 if d == 50 else 261
    x_all = mean + 1.2 * rng.normal(size=(n_max, d)) @ chol.T
    y = solve_triangular(chol, (x_all - mean).T, lower=True)
    want_all = np.sum(y**2, axis=0)
    for n in (1, 127, 261) + ((33000,) if d == 50 else ()):
        x = torch.from_numpy(x_all[:n]).cuda()
        out = torch.full((n, 2), 7.0, dtype=torch.float64, device='cuda')
        with dev.EvalCounters() as counters:
            _call(plain._lib.nb_neural_score, plain._h, x, out,
                  torch.cuda.current_stream())
        assert counters.read() == dict(outer_point_evals=0,
                                       ellipsoid_point_evals=n,
                                       emulator_point_evals=0)
        r2 = out[:, 0]
        print('d %d n %d: largest relative r2 error %.3g' % (
            d, n, np.max(np.abs(r2.cpu().numpy() - want_all[:n]) /
                         want_all[:n])))
        assert np.allclose(r2.cpu().numpy(), want_all[:n], rtol=1e-12,
                           atol=1e-13)
        assert torch.equal(out[:, 1], torch.zeros_like(r2))
        assert torch.equal(plain.neural_score(x)[0], r2)
        assert torch.equal(with_net.neural_score(x)[0], r2)


def union_of_three(d):
    """K = 3 overlapping members in d dimensions, the last one clipped by box
    limits (a mixture whose dimension 0 is a cube dimension; for d = 1 nothing
    but the cube), and 261 rows around them that leave [0, 1) in dimension 0."""
    from oracle import bounds_oracle as bo
    rng = np.random.default_rng(1700 + d)
    centres = 0.5 + rng.normal(size=(3, d)) * (0.1 / np.sqrt(d))
    centres[:, 0] = 0.9
    members, ells = [], []
    for j in range(3):
        b_mat = np.tril(rng.normal(size=(d, d)) * 0.02) + np.eye(d) * 0.3
        if j < 2:
            ells.append(bo.OEllipsoid.from_params(centres[j], b_mat))
            members.append(ells[-1])
            continue
        dim_cube = np.arange(d) == 0
        rest = None
        if d > 1:
            rest = bo.OEllipsoid.from_params(centres[j, 1:], b_mat[1:, 1:])
            ells.append(rest)
        members.append(bo.OMixture.from_params(dim_cube, rest))
    union = bo.OUnion.from_members(members, unit=False)
    # (distances from well inside to well outside; dimension 0 on its own
    # scale, so that rows pass x = 1 at any d)
    step = rng.normal(size=(261, d)) * (0.28 / np.sqrt(d))
    step[:, 0] = 0.1 * rng.normal(size=261)
    x = centres[rng.integers(3, size=261)] + \
        step * rng.uniform(0.5, 1.6, size=(261, 1))
    if d == 1:
        x = 0.9 + 0.3 * step / 0.1
    # rows whose r2 against some member lies within rounding of the surface
    edge = np.zeros(len(x), dtype=bool)
    for j, ell in enumerate(ells):
        cols = x if j < 2 else x[:, 1:]
        edge |= near_boundary(np.sum(ell.transform(cols)**2, axis=1), 1.0,
                              1e-12)
    return union, x, edge


@pytest.mark.parametrize('d', DIMS)
def test_member_count_every_tile_count(dev, d):
    """count mode: ``member_count`` equals the sum of ``contains`` of every
    member uploaded alone (integers, exact) and the oracle's overlap count
    (union.py:316-317) away from the members' surfaces; no unit-cube clip."""
    union, x, edge = union_of_three(d)
    assert edge.mean() < 1e-3
    b = upload(union)
    assert b.n_members == 3
    xd = torch.from_numpy(x).cuda()
    with dev.EvalCounters() as counters:
        count = b.member_count(xd)
    assert counters.read()['outer_point_evals'] == 3 * len(x)
    alone = sum(upload(m).contains(xd).to(torch.uint8) for m in union.bounds)
    assert count.dtype == torch.uint8 and torch.equal(count, alone)
    want = union.member_count(x)
    assert np.array_equal(count.cpu().numpy()[~edge], want[~edge])
    # every count occurs, rows outside the cube are counted, and the box
    # limits of the third member decide for some rows
    assert set(np.unique(want)) == {0, 1, 2, 3}
    outside = ~np.all((x >= 0) & (x < 1), axis=1)
    assert np.any(want[outside] > 0)
    if d > 1:
        last = union.bounds[2]
        assert np.any(last.ellipsoid.contains(x[:, 1:]) & ~last.contains(x))


def test_one_kernel_exports_run_the_two_stages(dev):
    """nb_contains, nb_accept (of a bound the fused kernel does not take),
    nb_contains_any and nb_first_containing keep their conventions -- masks of
    0 / 1, -1 for no bound, the flags byte -- on the two stages, and a second
    stream sharing the handles gets the same bytes."""
    from nautilus_amd import _lib
    from oracle import bounds_oracle as bo
    lib = _lib.load()
    g = load_golden('nautilusbound_D4')
    ob = nautilus_from_golden(g)
    b = upload(ob)
    n = 20000
    main = torch.cuda.current_stream()
    x = b.propose(5, 0, n)

    def u8():
        return torch.full((n,), 7, dtype=torch.uint8, device='cuda')

    mask = _call(lib.nb_contains, b._h, x, u8(), main)
    want = b.contains(x)
    assert 0.01 < float(want.float().mean()) < 0.99
    assert torch.equal(mask, want.to(torch.uint8))

    # two outer members and two neural bounds around the fixture's
    member, nb0 = ob.outer_bound.bounds[0], ob.neural_bounds[0]
    e0 = member.ellipsoid
    nb1 = nautilus_from_golden(g).neural_bounds[0]
    nb1.outer_bound = bo.OEllipsoid.from_params(nb0.outer_bound.c - 0.05,
                                                0.8 * nb0.outer_bound.B)
    nb1.score_predict_min = nb0.score_predict_min + 0.02
    outer = bo.OUnion.from_members(
        [member, bo.OMixture.from_params(
            member.dim_cube, bo.OEllipsoid.from_params(e0.c + 0.05,
                                                       0.9 * e0.B))],
        unit=True)
    b2 = upload(bo.ONautilus.from_parts(outer, [nb0, nb1]))
    assert b2.n_members == 2 and b2.n_neural == 2
    seed, offset = 9, 10**9 + 1
    x2 = b2.propose(seed, offset, n)
    before = dict(dev.DISPATCHES)
    staged = b2.accept(seed, offset, x2)
    assert dev.DISPATCHES['nb_cand_kernel'] == before['nb_cand_kernel'] + 1
    flags = _call(lib.nb_accept, b2._h, x2, u8(), main, seed, offset)
    assert torch.equal(flags, staged)
    assert len(torch.unique(flags)) == 3           # 0, kept, accepted

    empty = dev.DeviceBoundList([])
    assert torch.equal(_call(lib.nb_contains_any, empty._h, x, u8(), main),
                       torch.zeros(n, dtype=torch.uint8, device='cuda'))
    idx = torch.full((n,), 7, dtype=torch.int32, device='cuda')
    assert torch.equal(_call(lib.nb_first_containing, empty._h, x, idx, main),
                       torch.full_like(idx, -1))

    # the same handles from a second stream
    side = torch.cuda.Stream()
    side.wait_stream(main)
    with torch.cuda.stream(side):
        mask_side = _call(lib.nb_contains, b._h, x, u8(), side)
        flags_side = _call(lib.nb_accept, b2._h, x2, u8(), side, seed, offset)
    side.synchronize()
    assert torch.equal(mask_side, mask)
    assert torch.equal(flags_side, flags)
