"""The recipe of accept_cases.py against the oracle, on the CPU: at every
dimension of ``DIMS`` every decision of ``accept`` goes both ways, and hardly
a row lies within rounding of one.  test_accept_routes_gpu.py compares the
device with the oracle outside such rows only; this file is the check that
its exclusions cannot hide a failure."""

import numpy as np
import pytest

import accept_cases as ac


def test_dims_cover_every_instantiation():
    """40 dimensions: every (DT, KT1) of nb_eval_fast.hip's dispatch and every
    (DT, SMALL) of nb_cand.hip's (SMALL exists from DT 2 on)."""
    assert len(ac.DIMS) == len(set(ac.DIMS)) == 40
    assert ac.DIMS[:5] == [1, 4, 5, 15, 16] and ac.DIMS[-1] == 128
    fast = {ac.instantiation(d)['fast'] for d in ac.DIMS}
    assert fast == {(dt, dt + i) for dt in range(1, 9) for i in (0, 1)}
    cand = {(c['DT'], c['SMALL']) for c in
            (ac.instantiation(d)['cand'] for d in ac.DIMS)}
    assert cand == ({(dt, False) for dt in range(1, 9)} |
                    {(dt, True) for dt in range(2, 9)})


@pytest.mark.parametrize('k,m', [(1, 1), (3, 2)])
@pytest.mark.parametrize('d', ac.DIMS)
def test_every_decision_goes_both_ways(d, k, m):
    p = ac.proposals(d, k, m)
    n = ac.N_ROWS
    reach = np.any(p.reach, axis=0)
    shares = dict(cube=p.in_cube.mean(), reach=reach.mean(),
                  accept=p.accept.mean())
    assert shares['reach'] >= 0.05 and shares['accept'] >= 0.02, shares
    assert all(s <= 0.95 for s in shares.values()), shares
    # (a kept row that no emulator accepts, and one inside an ellipsoid whose
    # emulator says no)
    assert np.any(reach & ~p.accept) and np.any(p.keep & ~reach)
    if k > 1:
        dropped = p.in_cube & ~p.keep
        assert dropped.sum() >= 5 and dropped.mean() <= 0.95
        # ... of which the draw, not the cube, decided; rows that no member
        # contains are kept (union.py:318-319)
        assert np.all(p.k_cnt[dropped] >= 2)
        assert np.all(p.keep[p.in_cube & (p.k_cnt <= 1)])
        for reach_m in p.reach:            # every candidate list gets rows
            assert reach_m.mean() >= 0.02
    else:
        assert np.array_equal(p.keep, p.in_cube)
    assert (p.edge | p.edge_outer).sum() <= 2
    assert len(p.x) == n


@pytest.mark.parametrize('d', ac.DIMS)
def test_list_case(d):
    c = ac.list_case(d)
    assert len(c.obs) == 10 and c.inside[-1].all()
    any_in = c.inside[:-1].any(axis=0)
    assert 0.1 < any_in.mean() < 0.9
    for ob, row in zip(c.obs[:-1], c.inside[:-1]):
        assert row.any() and not row.all()
        if ob.neural_bounds:      # the outer bound alone does not decide
            xs = c.x if ob.shift is None else ob.shift.transform(c.x)
            assert np.any(ob.outer_bound.contains(xs) & ~row)
    assert c.edge.mean() < 1e-3
    # the bounds the candidate kernel treats differently are all there
    assert c.obs[1].shift is not None
    assert len(c.obs[3].neural_bounds) == 0
    assert len(c.obs[3].outer_bound.bounds) == 2
    assert c.obs[4].neural_bounds[0].emulator is None
    assert (d == 1) != hasattr(c.obs[5].outer_bound.bounds[0], 'dim_cube')
    assert len(c.obs[7].outer_bound.bounds) == 0
