"""The cases and the reference of mixture_cases.py, on the CPU: the table
reaches every instantiation of ``nb_mixture_loglike`` in both regimes, the
restated launcher agrees with the record sizes of nb_layout.h, the round
tables give three rounds, and the long double reference agrees with scipy and
holds an fp64 evaluation inside its bound -- so the device tests
(test_mixture_sweep_gpu.py) judge the kernel and nothing else."""

import numpy as np
import pytest
from scipy.special import logsumexp

import mixture_cases as mc
from nautilus_amd import device


def test_table_reaches_every_instantiation_in_both_regimes():
    assert len(mc.DIMS) == 56 == len(set(mc.DIMS))
    assert len(mc.CASES) == 112
    assert min(mc.DIMS) == 1 and max(mc.DIMS) == 128
    seen = {}
    for d, k in mc.CASES:
        dt, kl, small, tpw, resident, _ = device.mixture_launch_shape(d, k)
        seen.setdefault((dt, kl, small), set()).add(resident)
        assert dt == -(-d // 16)
        assert tpw == (4 if dt <= 2 else 2 if dt <= 4 else 1)
        assert kl == 2 * -(-d // 8)                # k-steps with real features
        assert (kl, small) == {
            'full': (4 * dt, False), 'small': (4 * dt - 2, True),
            'trimmed': (4 * dt - 2, False)}[mc.trim_class(d)]
    assert len(seen) == 24
    assert sorted(seen) == sorted(
        (dt, kl, small) for dt in range(1, 9)
        for kl, small in ((4 * dt, False), (4 * dt - 2, True),
                          (4 * dt - 2, False)))
    assert all(regimes == {True, False} for regimes in seen.values())
    # both parities of n_dim in every class at every DT
    for dt in range(1, 9):
        for name in ('small', 'trimmed', 'full'):
            par = {d % 2 for d in mc.DIMS
                   if -(-d // 16) == dt and mc.trim_class(d) == name}
            assert par == {0, 1}


def test_component_counts_sit_either_side_of_the_boundary():
    for d in mc.DIMS:
        assert device.mixture_launch_shape(d, mc.k_resident(d))[4]
        assert not device.mixture_launch_shape(d, mc.k_streamed(d))[4]
        assert device.mixture_launch_shape(d, mc.k_streamed(d) - 1)[4]
        assert 2 <= mc.k_resident(d) <= 3


def test_largest_resident_count_per_tile_count():
    want = [53, 22, 12, 7, 5, 3, 2, 2]
    for dt in range(1, 9):
        for d in range(16 * dt - 15, 16 * dt + 1):
            assert mc.largest_resident(d) == want[dt - 1]
            for k in (1, 2):
                assert device.mixture_launch_shape(d, k)[4]
        # nb_layout.h, nb_mixture_record
        tiles = dt * (dt + 1) // 2
        assert device.mixture_record(dt) == tiles * 256 + \
            (128 if 16 * dt + 1 <= 128 else 256)
        assert want[dt - 1] == 160 * 1024 // (8 * device.mixture_record(dt))


def test_launch_shape_rounds_and_errors():
    # (dt, kl, small, tpw, resident, points_per_round)
    assert device.mixture_launch_shape(1, 1) == (1, 2, True, 4, True, 262144)
    assert device.mixture_launch_shape(50, 4) == (4, 14, True, 2, True, 65536)
    assert device.mixture_launch_shape(50, 3) == (4, 14, True, 2, True, 131072)
    assert device.mixture_launch_shape(50, 64) == (
        4, 14, True, 2, False, 65536)
    assert device.mixture_launch_shape(128, 2) == (
        8, 32, False, 1, True, 32768)
    assert device.mixture_launch_shape(128, 3) == (
        8, 32, False, 1, False, 32768)
    assert device.mixture_launch_shape(22, 4096)[4:] == (False, 131072)
    for d, k in ((0, 1), (129, 1), (3, 0), (3, 4097), (-1, 1)):
        with pytest.raises(ValueError):
            device.mixture_launch_shape(d, k)


def test_round_tables_give_three_rounds_with_a_ragged_last_one():
    forms = set()
    for d, k in mc.ROUND_CASES:
        dt, _, _, tpw, resident, per_round = device.mixture_launch_shape(d, k)
        forms.add((resident, tpw, k % 2 if not resident else None))
        assert 5 <= d % 16 <= 8                    # the "trimmed" class
        n = mc.round_rows(d, k)
        per = per_round // (16 * tpw)
        assert mc.rounds_of(d, k, n) == [per, per, 2]
        assert n % (16 * tpw) == 5                 # the last group has 5 rows
        assert mc.rounds_of(d, k, mc.ROUND_BASE) == [-(-mc.ROUND_BASE //
                                                       (16 * tpw))]
        # shifted by one row the launch keeps its three rounds
        assert mc.rounds_of(d, k, n - 1) == [per, per, 2]
        assert n * d * 8 < 120e6
    assert forms == {(True, t, None) for t in (4, 2, 1)} | \
        {(False, t, p) for t in (4, 2, 1) for p in (0, 1)}


@pytest.mark.parametrize('d, k, overlap', [(1, 2, False), (3, 5, False),
                                           (22, 4, False), (22, 4, True),
                                           (54, 3, True)])
def test_reference_agrees_with_scipy(d, k, overlap):
    """scipy factors the covariance on its own (an eigendecomposition), so
    the agreement is that of two routes to the same number: the band of the
    existing tests."""
    seed = 100 * d + k
    means, covs, w = (mc.overlapping if overlap else mc.problem)(d, k, seed)
    x = mc.points(means, covs, w, seed, 100)
    chol_inv, log_coef = mc.table_arrays(means, covs, w)
    values, bound, terms, term_bound = mc.reference(means, chol_inv, log_coef,
                                                    x)
    assert values.dtype == bound.dtype == np.float64
    assert values.shape == bound.shape == (200,)
    assert terms.shape == term_bound.shape == (k, 200)
    assert terms.dtype == np.longdouble
    sp = mc.scipy_terms(means, covs, w, x)
    assert np.allclose(np.asarray(terms, float), sp, rtol=mc.RTOL,
                       atol=mc.ATOL)
    assert np.allclose(values, logsumexp(sp, axis=0), rtol=mc.RTOL,
                       atol=mc.ATOL)
    assert np.all(bound > 0) and np.all(term_bound > 0)


def test_reference_logsumexp_in_small_cases():
    """Components and points whose terms are known in closed form."""
    means = np.array([[0.0, 0.0], [3.0, 4.0]])
    chol_inv = np.stack([np.eye(2), np.eye(2)])
    log_coef = np.array([0.0, np.log(3.0)])
    x = np.array([[0.0, 0.0], [3.0, 4.0], [1.5, 2.0]])
    values, bound, terms, tb = mc.reference(means, chol_inv, log_coef, x)
    want = np.array([[0.0, -12.5, -3.125],
                     [np.log(3.0) - 12.5, np.log(3.0), np.log(3.0) - 3.125]])
    assert np.allclose(np.asarray(terms, float), want, rtol=0, atol=1e-15)
    assert np.allclose(values, [np.log1p(3 * np.exp(-12.5)),
                                np.log(3 + np.exp(-12.5)),
                                np.log(4.0) - 3.125], rtol=0, atol=1e-15)
    assert np.all(bound < 1e-13)
    label, clear = mc.clear_labels(terms, tb)
    assert label.tolist() == [0, 1, 1] and clear.all()
    # an exact tie is never clear; one component always is
    tie = np.array([[1.0, 2.0], [1.0, 0.0]], np.longdouble)
    label, clear = mc.clear_labels(tie, np.full((2, 2), 1e-12))
    assert clear.tolist() == [False, True] and label[1] == 0
    assert mc.clear_labels(tie[:1], np.ones((1, 2)))[1].all()


def test_terms_far_below_the_largest_do_not_set_the_bound():
    means = np.zeros((2, 1))
    chol_inv = np.ones((2, 1, 1))
    x = np.array([[1e3]])
    _, near, _, tb = mc.reference(means, chol_inv, np.array([0.0, -10.0]), x)
    _, far, _, tb_far = mc.reference(means, chol_inv,
                                     np.array([0.0, -5e6]), x)
    assert near[0] >= tb.max()
    assert tb_far[1, 0] > 1.5 * tb_far[0, 0] and far[0] < tb_far[1, 0]
    assert far[0] >= tb_far[0, 0]


def test_fold_bound_grows_with_the_count():
    b = [mc.fold_bound(k, 0.0) for k in (1, 2, 53, 4096)]
    assert all(x < y for x, y in zip(b, b[1:]))
    assert b[0] >= 2 * mc.EPS and b[-1] < 1e-11
    assert mc.fold_bound(3, -1e6) >= mc.EPS * 1e6


def _used(d, k, overlap=False):
    means, chol_inv, log_coef, x = mc.case(d, k, overlap)
    values, bound, terms, term_bound = mc.case_reference(d, k, overlap)
    got, got_terms = mc.twin(means, chol_inv, log_coef, x)
    used_t = np.abs(got_terms - terms).astype(float) / term_bound
    used = np.abs(got - values) / bound
    label, clear = mc.clear_labels(terms, term_bound)
    return used_t.max(), used.max(), label, clear, got_terms


@pytest.mark.parametrize('d, k', mc.CASES,
                         ids=['%d-%d' % c for c in mc.CASES])
def test_fp64_twin_inside_the_bound_and_labels_clear(d, k):
    means, chol_inv, log_coef, x = mc.case(d, k)
    assert x.shape == (2 * mc.N_HALF, d) and x.shape[0] % 16 != 0
    assert means.shape == (k, d) and chol_inv.shape == (k, d, d)
    assert not x.flags.writeable
    used_t, used, label, clear, got_terms = _used(d, k)
    assert used_t <= 1.0 and used <= 1.0, (used_t, used)
    assert np.mean(~clear) <= 1e-3
    assert np.array_equal(np.argmax(got_terms, axis=0)[clear], label[clear])
    if k > 1:                       # more than one component owns rows
        assert len(np.unique(label)) > 1


@pytest.mark.parametrize('dt', range(2, 9))
def test_overlapping_cases_stay_clear(dt):
    """At n_dim = 16 (DT - 1) + 6 with the shared covariance of
    ``overlapping`` and a count on either side of the boundary."""
    d = 16 * (dt - 1) + 6
    for k in (mc.largest_resident(d), mc.k_streamed(d)):
        used_t, used, label, clear, got_terms = _used(d, k, True)
        assert used_t <= 1.0 and used <= 1.0, (k, used_t, used)
        assert np.mean(~clear) <= 1e-3
        assert np.array_equal(np.argmax(got_terms, axis=0)[clear],
                              label[clear])
