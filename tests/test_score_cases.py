"""The recipe of score_cases.py against its floors, on the CPU: the long
double reference is finer than fp64 and the fp64 oracle sits an ulp or two
from it (the unit test_score_rows_gpu.py counts the device's error in), every
case has rows on both sides of every rim, the periodic rows wrap, the index
lists are what their names say, every (n_dim, neural bound) pair of the
staged-route cases has rows whose acceptance one emulator decides alone, and
an uploaded threshold can be put on any score."""

import numpy as np
import pytest

import accept_cases as ac
import score_cases as sc

CASES = ([('per_dim', (d,)) for d in ac.DIMS] +
         [('width', de) for de in sc.WIDTH] +
         [('periodic', (d,)) for d in sc.PERIODIC])


def _ids(case):
    return '%s-%s' % (case[0], '-'.join(str(a) for a in case[1]))


def test_long_double_is_finer_than_fp64():
    assert np.finfo(np.longdouble).nmant >= 63


def test_case_lists():
    assert sc.WIDTH == ((5, 1), (50, 4), (80, 8), (100, 8), (128, 1),
                        (128, 4))
    assert sc.PERIODIC == (1, 5, 17, 64, 128)
    assert all(d in ac.DIMS for d in sc.PERIODIC + sc.LONG_DIMS)
    # layer 1 in one stage and in two K chunks (nb_eval_fast.hip: from n_dim
    # 80 on), list tiles per wavefront (accept_cases.instantiation)
    assert {d >= 80 for d, _ in sc.WIDTH} == {False, True}
    assert {ac.instantiation(d)['cand']['T_list'] for d, _ in sc.WIDTH} == {
        1, 2}
    assert {e for _, e in sc.WIDTH} >= {1, 8}
    edge = sc.tile_edge_dims()
    assert len(edge) == 16 and all(d in ac.DIMS for d in edge)
    assert {ac.instantiation(d)['fast'] for d in edge} == {
        ac.instantiation(d)['fast'] for d in ac.DIMS}


@pytest.mark.parametrize('case', CASES, ids=_ids)
def test_reference_and_rows(case):
    c = getattr(sc, case[0])(*case[1])
    d = c.d
    assert c.x.shape == (sc.N_ROWS, d) and sc.N_ROWS == 2 * 128 + 37
    assert np.all(np.isfinite(c.x))
    assert len(np.unique(c.x, axis=0)) == sc.N_ROWS
    n_m = dict(per_dim=2, width=3, periodic=1)[case[0]]
    assert len(c.neural) == n_m
    assert all(len(nb.emulator.networks) == c.E for nb in c.neural)
    refs = sc.reference(case[0], *case[1])
    assert len(refs) == n_m
    for m, (nb, (ref, (e_r2, e_score))) in enumerate(zip(c.neural, refs)):
        # (the device reads the lower triangle of B_inv alone)
        assert np.array_equal(nb.outer_bound.B_inv,
                              np.tril(nb.outer_bound.B_inv))
        assert ref[0].dtype == ref[1].dtype == np.longdouble
        assert ref[0].shape == ref[1].shape == (sc.N_ROWS,)
        print('%s m=%d: fp64 oracle against long double: r2 %.3g relative, '
              'score %.3g absolute' % (c.name, m, e_r2, e_score))
        assert 0.0 < e_r2 < 2.0**-50 and 0.0 < e_score < 2.0**-50
        r2 = ref[0].astype(float)
        assert (r2 < 1).sum() >= 64 and (r2 > 1).sum() >= 64
        assert (r2 > 3.9).sum() >= 1               # far outside
    xs = c.x if c.shift is None else c.shift.transform(c.x)
    out_of_cube = np.any((xs < 0) | (xs >= 1), axis=1)
    if case != ('periodic', (1,)):         # (its one feature is periodic)
        assert out_of_cube.sum() >= 3
    if c.shift is not None:
        per = c.shift.periodic
        assert list(per) == sorted({0, d - 1})
        assert np.all((c.x[:, per] >= 0) & (c.x[:, per] < 1))
        wraps = sc.wraps(c)
        assert wraps.sum() >= 3
        assert np.all(np.minimum(xs[:, per], 1.0 - xs[:, per]) > 1e-9)


def test_index_lists():
    n = sc.N_ROWS
    lists = sc.index_lists()
    assert set(lists) == {'identity', 'reversed', 'permutation', 'thrice',
                          'one_row', 'every_third'} | {
                              'prefix_%d' % k for k in sc.PREFIXES}
    assert sc.PREFIXES == (1, 15, 16, 17, 127, 128, 129)
    for a in lists.values():
        assert a.dtype == np.int64 and a.ndim == 1
        assert a.min() >= 0 and a.max() < n
    assert np.array_equal(lists['identity'], np.arange(n))
    assert np.array_equal(lists['reversed'], np.arange(n - 1, -1, -1))
    perm = lists['permutation']
    assert np.array_equal(np.sort(perm), np.arange(n))
    assert not np.array_equal(perm, np.arange(n))
    assert np.array_equal(np.bincount(lists['thrice'], minlength=n),
                          np.full(n, 3))
    assert len(lists['one_row']) == n and len(set(lists['one_row'])) == 1
    assert np.array_equal(lists['every_third'], np.arange(n)[::3])
    for k in sc.PREFIXES:
        assert np.array_equal(lists['prefix_%d' % k], np.arange(k))
    long = sc.long_list()
    # (256 workgroups at the most, 128 rows a pass: some take a second pass)
    assert len(long) == 32901 > 256 * 128 and long.dtype == np.int64
    assert np.array_equal(long, np.arange(32901) % n)
    source, idx = sc.wide_list()
    assert len(source) == 1000 and len(idx) == n
    assert source.min() >= 0 and source.max() < n
    assert idx.min() == 0 and idx.max() == 999
    assert idx[0] == 999 and idx[-1] == 0


# (d, m) pairs of the (d, 3, 2) cases in which no row's acceptance is decided
# by emulator m alone, with the reason; at most two may be listed
NO_PIVOTS = {}


def test_pivot_rows():
    """Rows kept by the outer union, inside ellipsoid m and not accepted
    through the other neural bound: the rows on which a wrong score of
    emulator m changes the flag."""
    assert len(NO_PIVOTS) <= 2
    counts = {}
    for d in ac.DIMS:
        p = ac.proposals(d, 3, 2)
        for m, piv in enumerate(sc.oracle_pivots(d)):
            counts[d, m] = int(piv.sum())
            assert np.all(p.keep[piv] & p.inside[m][piv])
            if (d, m) not in NO_PIVOTS:
                # ... and both ways: some accepted, some not
                assert 0 < p.accept[piv].sum() < piv.sum(), (d, m)
    print('pivot rows per (d, m): %s' % counts)
    assert len(counts) == 80
    few = {key for key, n in counts.items() if n < sc.MIN_PIVOTS}
    assert few == set(NO_PIVOTS), few
    # n_dim 1, bound 1: its interval lies inside bound 0's, no row reaches it
    # alone -- its pivots reach both and fail bound 0's threshold
    p = ac.proposals(1, 3, 2)
    piv = sc.oracle_pivots(1)[1]
    assert not np.any(p.reach[1] & ~p.reach[0])
    assert piv.sum() >= sc.MIN_PIVOTS and np.all(p.reach[0][piv])


def test_threshold_search():
    """``predict_min_for``: float(min) - 1e-9, the subtraction the upload
    makes, gives the target exactly -- for targets over [-4, 4], on scores of
    the cases and their neighbours, and within a few steps of target +
    1e-9."""
    rng = np.random.default_rng(3)
    c = sc.per_dim(5)
    scores = sc.oracle_scores(c.neural[0], c.x)[1]
    targets = np.concatenate([
        rng.uniform(-4.0, 4.0, size=4000), scores,
        np.nextafter(scores, -np.inf), [-4.0, 3.999, 0.75, -0.5, -1.0,
                                        np.nextafter(-1.0, 0.0)]])
    for t in targets:
        s = sc.predict_min_for(t)
        assert isinstance(s, float) and float(s) - 1e-9 == t
        assert abs(s - (t + 1e-9)) <= 8 * np.spacing(abs(t) + 1e-9)
    # where min has the coarser grid only every other target exists
    with pytest.raises(ValueError):
        for t in 1.0 - 2.0**-53 * np.arange(1, 5):
            sc.predict_min_for(t)
    ob = sc.with_threshold(c.ob, 1, scores[0])
    assert ob.neural_bounds[1].score_predict_min - 1e-9 == scores[0]
    assert ob.neural_bounds[0] is c.ob.neural_bounds[0]
    assert ob.neural_bounds[1].emulator is c.ob.neural_bounds[1].emulator
    assert c.ob.neural_bounds[1].score_predict_min != \
        ob.neural_bounds[1].score_predict_min
