"""``GaussianProcessSeriesLikelihood`` with a sum of kernel terms, without a
GPU: the numpy twin of the recursion of nb_gps_filter.h against a dense
Cholesky factorisation of the defining covariance in ``np.longdouble`` and
against LAPACK on the same matrix, the invariance under the order of the
terms, switched-off terms, the NaN rules and what the constructor refuses.
The problems, the truth and the tolerance of the device tests
(test_gps_terms_gpu.py) live here as well."""

import functools
import itertools
import pickle

import numpy as np
import pytest
import torch

from nautilus_amd import (GaussianProcessLikelihood,
                          GaussianProcessSeriesLikelihood)
from nautilus_amd.likelihoods import (GPS_KERNELS, GPS_MAX_STATES,
                                      GPS_MAX_TERMS, GPS_STATES)
from test_gps_likelihood import (DENSE_N, DENSE_P, EPS, LD, budget,
                                 cholesky_value, correlation, identity, make)

# the 10 pairs and 13 triples, names in the order of their kernel codes
COMBOS = tuple(
    c for k in (2, 3)
    for c in itertools.combinations_with_replacement(GPS_KERNELS, k)
    if sum(GPS_STATES[name] for name in c) <= GPS_MAX_STATES)


def name_of(kernel):
    return '+'.join(kernel)


def width(kernel):
    return sum(3 if name == 'sho' else 2 for name in kernel) + 1


def columns(kernel):
    """First column of every term's (a, l[, q]) in a row of h."""
    return list(np.cumsum([0] + [3 if name == 'sho' else 2
                                 for name in kernel])[:-1])


@functools.lru_cache(maxsize=32)
def problem(p, n, kernel):
    """t, data, sigma, n model rows and their hyper-parameters, deterministic
    from the arguments: t sorted uniform on [0, 10] with one pair of equal
    neighbours (from P = 2 on), sigma uniform in [0.1, 1], m the data plus
    N(0, 0.5^2) and per term a log-uniform in [1e-1, 1e1], l in 10^[-1.5, 1]
    and, for 'sho', q uniform in [0.51, 50]; s in [1e-4, 1e-1].  Nobody writes
    to the result."""
    rng = np.random.default_rng(
        [p, n, 77] + [GPS_KERNELS.index(name) for name in kernel])
    t = np.sort(rng.uniform(0, 10, size=p))
    if p > 1:
        t[p // 2] = t[p // 2 - 1]
    sigma = rng.uniform(0.1, 1, size=p)
    d = rng.normal(size=p)
    m = d + 0.5 * rng.normal(size=(n, p))
    cols = []
    for name in kernel:
        cols += [10.0**rng.uniform(-1, 1, size=n),
                 10.0**rng.uniform(-1.5, 1, size=n)]
        if name == 'sho':
            cols.append(rng.uniform(0.51, 50, size=n))
    cols.append(10.0**rng.uniform(-4, -1, size=n))
    h = np.stack(cols, axis=1)
    assert h.shape == (n, width(kernel))
    for arr in (t, d, sigma, m, h):
        arr.setflags(write=False)
    return t, d, sigma, m, h


@functools.lru_cache(maxsize=None)
def truth(p, n, kernel):
    """The twin in ``np.longdouble`` on ``problem``."""
    t, d, sigma, m, h = problem(p, n, kernel)
    out = make(t, d, sigma, kernel).numpy_from_model(m, h, dtype=LD)
    assert out.dtype == LD and np.all(np.isfinite(out))
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def twin64(p, n, kernel):
    t, d, sigma, m, h = problem(p, n, kernel)
    out = make(t, d, sigma, kernel).numpy_from_model(m, h)
    assert out.dtype == np.float64 and np.all(np.isfinite(out))
    out.setflags(write=False)
    return out


def case_budget(p, n, kernel):
    """The device's tolerance (``budget`` of test_gps_likelihood.py: eight
    times the float64 twin's own error, at least 64 eps |truth|)."""
    return budget(twin64(p, n, kernel), truth(p, n, kernel))


def covariance(kernel, dist, h, ty):
    """sum_i a_i rho_i(dist / l_i) + s I of every row of h, (n, P, P)."""
    total = None
    for name, col in zip(kernel, columns(kernel)):
        a, l = (h[:, col + i].astype(ty)[:, None, None] for i in range(2))
        q = h[:, col + 2].astype(ty)[:, None, None] if name == 'sho' else None
        term = a * correlation(name, dist * (1 / l), q)
        total = term if total is None else total + term
    return total + np.eye(dist.shape[0], dtype=ty) * \
        h[:, -1].astype(ty)[:, None, None]


def dense_truth(like, m, h):
    """Long-double dense Cholesky of the defining K; the times are the
    running sums of the float64 steps the filter reads, exact in long
    double."""
    tt = np.cumsum(like._dt.astype(LD))
    k = covariance(like.kernel, np.abs(tt[:, None] - tt[None, :]), h, LD)
    k += np.eye(len(tt), dtype=LD) * like._sigma2.astype(LD)
    return cholesky_value(k, m.astype(LD) - like.data.astype(LD))


def dense_float64(like, t, d, sigma, m, h):
    """LAPACK on the same K, through the dense class's numpy path."""
    dense = GaussianProcessLikelihood(identity, t, d, sigma, cov='full',
                                      normalised=False)
    return dense.numpy_from_model(
        m, covariance(like.kernel, dense.dist, h, np.float64))


def test_the_combinations():
    assert len(COMBOS) == 23
    assert len([c for c in COMBOS if len(c) == 2]) == 10
    assert max(width(c) for c in COMBOS) == 10
    assert ('sho', 'sho', 'sho') in COMBOS
    assert ('matern52', 'matern52') in COMBOS
    assert ('exp', 'matern32', 'matern52') in COMBOS


@pytest.mark.parametrize('kernel', COMBOS, ids=name_of)
@pytest.mark.parametrize('p', DENSE_P)
def test_twin_against_dense_cholesky(p, kernel):
    t, d, sigma, m, h = problem(p, DENSE_N, kernel)
    like = make(t, d, sigma, kernel)
    want = dense_truth(like, m, h)
    got = truth(p, DENSE_N, kernel)
    rel = float(np.max(np.abs(got - want) / np.abs(want)))
    got64 = twin64(p, DENSE_N, kernel)
    lapack = dense_float64(like, t, d, sigma, m, h)
    assert np.all(np.isfinite(got64)) and np.all(np.isfinite(lapack))
    err = float(np.max(np.abs(got64.astype(LD) - want)))
    err_dense = float(np.max(np.abs(lapack.astype(LD) - want)))
    floor = float(np.max(64 * EPS * np.abs(want)))
    print('P = %d, %s: long-double twin - dense Cholesky %.2g relative; '
          'float64 twin error %.3g, dense LAPACK error %.3g, floor %.3g, '
          'ratio %.3g' % (p, name_of(kernel), rel, err, err_dense, floor,
                          err / max(err_dense, floor)))
    assert rel <= 1e-14
    assert err <= 8 * max(err_dense, floor)


def permuted(kernel, h, perm):
    """The names in the order ``perm`` with their columns (s stays last)."""
    cols = columns(kernel)
    take = []
    for i in perm:
        take += range(cols[i], cols[i] + (3 if kernel[i] == 'sho' else 2))
    return tuple(kernel[i] for i in perm), h[:, take + [h.shape[1] - 1]]


@pytest.mark.parametrize('kernel', COMBOS, ids=name_of)
def test_the_order_of_the_terms_changes_no_bit(kernel):
    t, d, sigma, m, h = problem(16, 5, kernel)
    want = twin64(16, 5, kernel)
    seen = set()
    for perm in itertools.permutations(range(len(kernel))):
        other, h2 = permuted(kernel, h, perm)
        # equal names keep their order: otherwise it is another problem
        if any(other[i] == other[j] and perm[i] > perm[j]
               for i in range(len(perm)) for j in range(i + 1, len(perm))):
            continue
        seen.add(other)
        like = make(t, d, sigma, other)
        assert like.kernel == other
        assert np.array_equal(like.numpy_from_model(m, h2), want), other
        # a list is a tuple
        assert np.array_equal(
            make(t, d, sigma, list(other)).numpy_from_model(m, h2), want)
    assert len(seen) == len(set(itertools.permutations(kernel)))


def without(kernel, h, i):
    perm = [j for j in range(len(kernel)) if j != i]
    return permuted(kernel, h, perm)


@pytest.mark.parametrize('kernel', [c for c in COMBOS if len(c) == 3],
                         ids=name_of)
def test_a_term_with_a_zero_is_switched_off_bit_for_bit(kernel):
    """Against the composite without the term: the same bits."""
    t, d, sigma, m, h = problem(40, 6, kernel)
    for i in range(3):
        h0 = h.copy()
        h0[:, columns(kernel)[i]] = 0.0
        got = make(t, d, sigma, kernel).numpy_from_model(m, h0)
        other, h2 = without(kernel, h0, i)
        want = make(t, d, sigma, other).numpy_from_model(m, h2)
        assert np.all(np.isfinite(want))
        assert np.array_equal(got, want), (kernel, i)


@pytest.mark.parametrize('kernel', [c for c in COMBOS if len(c) == 2],
                         ids=name_of)
def test_a_pair_with_a_zero_is_the_single_term(kernel):
    """Against the string path, whose G00 has another form: rtol 1e-13."""
    t, d, sigma, m, h = problem(40, 6, kernel)
    for i in range(2):
        h0 = h.copy()
        h0[:, columns(kernel)[i]] = 0.0
        got = make(t, d, sigma, kernel).numpy_from_model(m, h0)
        (name,), h2 = without(kernel, h0, i)
        # (a, l[, q], s) -> the single term's (a, l, s[, q])
        h1 = h2[:, [0, 1, 3, 2]] if name == 'sho' else h2
        want = make(t, d, sigma, name).numpy_from_model(m, h1)
        assert np.allclose(got, want, rtol=1e-13, atol=0), (kernel, i)


def test_two_halves_of_an_exponential():
    t, d, sigma, m, h = problem(40, 6, ('exp', 'exp'))
    h2 = h.copy()
    h2[:, 0] = h2[:, 2] = 0.5 * h[:, 0]
    h2[:, 3] = h[:, 1]
    got = make(t, d, sigma, ('exp', 'exp')).numpy_from_model(m, h2)
    want = make(t, d, sigma, 'exp').numpy_from_model(m, h[:, [0, 1, 4]])
    assert np.allclose(got, want, rtol=1e-13, atol=0)


@pytest.mark.parametrize('kernel', COMBOS, ids=name_of)
def test_white_noise_is_a_sum_of_normal_log_densities(kernel):
    t, d, sigma, m, h = problem(40, 6, kernel)
    h = h.copy()
    h[:, columns(kernel)] = 0.0
    got = make(t, d, sigma, kernel, normalised=True).numpy_from_model(m, h)
    v = sigma**2 + h[:, -1:]
    want = -0.5 * np.sum((m - d)**2 / v + np.log(2 * np.pi * v), axis=1)
    assert np.allclose(got, want, rtol=1e-13, atol=0)


# ---------------------------------------------------------------- the NaN rules

BAD_A = (-1.0, np.nan, np.inf)
BAD_L = (0.0, -2.0, np.nan, np.inf)
BAD_Q = (0.5, 0.2, -1.0, np.nan, np.inf)
BAD_S = (-1e-3, np.nan, np.inf)


def bad_hyper(kernel):
    """(column, value) of every cause of a NaN row among the
    hyper-parameters: every column of every term, and s."""
    bad = []
    for name, col in zip(kernel, columns(kernel)):
        bad += [(col, v) for v in BAD_A] + [(col + 1, v) for v in BAD_L]
        if name == 'sho':
            bad += [(col + 2, v) for v in BAD_Q]
    return bad + [(width(kernel) - 1, v) for v in BAD_S]


@pytest.mark.parametrize('kernel', COMBOS, ids=name_of)
def test_nan_rules_of_the_twin(kernel):
    bad = bad_hyper(kernel)
    n = len(bad) + 5
    t, d, sigma, m, h = problem(20, n, kernel)
    like = make(t, d, sigma, kernel)
    clean = like.numpy_from_model(m, h)
    assert np.all(np.isfinite(clean))
    m2, h2 = m.copy(), h.copy()
    rows = []
    for i, (col, value) in enumerate(bad):
        h2[i, col] = value
        rows.append(i)
    for i, col, value in zip(range(len(bad), len(bad) + 3), (0, 7, 19),
                             (np.nan, np.inf, -np.inf)):
        m2[i, col] = value
        rows.append(i)
    got = like.numpy_from_model(m2, h2)
    assert np.all(np.isnan(got[rows]))
    rest = np.setdiff1d(np.arange(n), rows)
    assert len(rest) == 2 and np.array_equal(got[rest], clean[rest])
    # a_i = 0 is legal, one at a time and all at once
    for cols in [[c] for c in columns(kernel)] + [columns(kernel)]:
        h3 = h.copy()
        h3[:, cols] = 0.0
        assert np.all(np.isfinite(like.numpy_from_model(m, h3)))
    # a repeated time without any noise is unspecified: NaN or finite, and
    # the other rows keep their bits
    bare = make(t, d, None, kernel)
    h4 = h.copy()
    h4[::2, -1] = 0.0
    with_noise = bare.numpy_from_model(m, h)
    got = bare.numpy_from_model(m, h4)
    assert not np.any(np.isinf(got))
    assert np.array_equal(got[1::2], with_noise[1::2])


# ------------------------------------------------------------- what is refused

def test_constructor_refuses_bad_kernels():
    t = np.linspace(0, 1, 5)
    d = np.arange(5.0)

    def new(kernel):
        return GaussianProcessSeriesLikelihood(identity, t, d, kernel=kernel)

    assert new(('sho', 'sho', 'matern32')).kernel == ('sho', 'sho', 'matern32')
    assert new(['exp', 'sho']).kernel == ('exp', 'sho')
    assert new('sho').kernel == 'sho'
    for kernel in COMBOS:
        assert new(kernel)._width == width(kernel)
    with pytest.raises(ValueError, match="kernel='sho', the string"):
        new(('sho',))
    with pytest.raises(ValueError, match="kernel='exp', the string"):
        new(['exp'])
    limits = 'at most 3 terms and at most 6 states'
    for kernel in (('exp',) * 4, ('exp', 'exp', 'sho', 'sho'),
                   ('matern52', 'matern52', 'exp'),
                   ('matern32', 'matern52', 'sho'),
                   ('sho', 'matern52', 'sho'), ()):
        with pytest.raises(ValueError, match=limits):
            new(kernel)
    for kernel in (('exp', 'periodic'), ('periodic', 'exp', 'exp', 'exp'),
                   ('exp', None), ('exp', ('sho', 'sho')), None, 3):
        with pytest.raises(ValueError, match='kernel must be one of'):
            new(kernel)
    for kernel in (('exp', 'sqexp'), ['sqexp', 'sho', 'sho'], ('sqexp',)):
        with pytest.raises(ValueError, match='no finite state'):
            new(kernel)
    assert (GPS_MAX_TERMS, GPS_MAX_STATES) == (3, 6)
    assert GPS_STATES == {'exp': 1, 'matern32': 2, 'matern52': 3, 'sho': 2}


def test_model_outputs_are_checked():
    kernel = ('exp', 'sho')
    t, d, sigma, m, h = problem(6, 4, kernel)
    like = make(t, d, sigma, kernel)
    assert h.shape == (4, 6)
    with pytest.raises(ValueError, match=r'shape \(n, 6\)'):
        like.numpy_from_model(m[:, :5], h)
    with pytest.raises(ValueError, match=r'shape \(4, 6\)'):
        like.numpy_from_model(m, h[:3])
    with pytest.raises(ValueError, match=r'shape \(4, 6\)'):
        like.numpy_from_model(m, h[:, :5])
    with pytest.raises(ValueError, match=r'shape \(4, 6\)'):
        like.numpy_from_model(m, np.concatenate([h, h[:, :1]], axis=1))
    with pytest.raises(ValueError, match='both'):
        like.from_model(torch.from_numpy(m), h)
    with pytest.raises(ValueError, match='float64'):
        like.from_model(torch.from_numpy(m), torch.from_numpy(h).float())
    with pytest.raises(ValueError, match=r'shape \(4, 6\)'):
        like.from_model(torch.from_numpy(m), torch.from_numpy(h)[:, :4])


def pair_model(x):
    return x[:, :6], x[:, 6:]


def test_pickle_round_trip_and_numpy_call():
    kernel = ('sho', 'exp', 'sho')
    t, d, sigma, m, h = problem(6, 4, kernel)
    like = GaussianProcessSeriesLikelihood(pair_model, t, d, sigma,
                                           kernel=list(kernel))
    like._tables[0] = object()                   # stands for a device handle
    other = pickle.loads(pickle.dumps(like))
    assert other._tables == {} and like._tables
    assert other.kernel == kernel and other.n_data == 6
    assert other._slots == like._slots == (('exp', 3), ('sho', 0), ('sho', 5))
    x = np.concatenate([m, h], axis=1)
    want = like.numpy_from_model(m, h)
    assert np.all(np.isfinite(want))
    assert np.array_equal(other.numpy(x), want)
    assert np.array_equal(like.numpy(x), want)
    raw = make(t, d, sigma, kernel)
    assert np.allclose(want, like.log_norm + raw.numpy_from_model(m, h),
                       rtol=4 * EPS, atol=0)


def test_constants_repeat_the_header():
    import os
    from nautilus_amd import device
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, 'include', 'nautilus_hip.h')).read()
    assert '#define NB_GPS_MAX_TERMS %d\n' % GPS_MAX_TERMS in header
    assert '#define NB_GPS_MAX_STATES %d\n' % GPS_MAX_STATES in header
    assert '#define NB_ABI_VERSION 6\n' in header
    for kernel in COMBOS + GPS_KERNELS:
        assert device.gps_width(kernel) == (
            width(kernel) if isinstance(kernel, tuple)
            else 4 if kernel == 'sho' else 3)
    from nautilus_amd import _lib
    assert 'nb_gps_create_terms' in _lib.exported_symbols()
