"""``GaussianProcessSeriesLikelihood`` without a GPU: the numpy twin of the
O(P) filter against a dense Cholesky factorisation of the defining covariance
in ``np.longdouble`` and against the dense class's own numpy path, its limits
(white noise, a gap beyond the cap), the NaN rules, and what the constructor
and ``from_model`` refuse.  The problems, the truth and the tolerance of the
device tests (test_gps_likelihood_gpu.py) live here as well."""

import functools
import pickle

import numpy as np
import pytest
import torch

from nautilus_amd import (GaussianNoiseLikelihood, GaussianProcessLikelihood,
                          GaussianProcessSeriesLikelihood)
from nautilus_amd.likelihoods import (GPS_CAP, GPS_KERNELS, N_GPS_MAX,
                                      gp_correlation, sho_correlation)

EPS = 2.0**-52
LD = np.longdouble
SHARED = ('exp', 'matern32', 'matern52')        # also in the dense class
DENSE_P = (1, 2, 16, 64, 128)
DENSE_N = 8


def identity(x):
    return x


def make(t, d, sigma, kernel, normalised=False):
    return GaussianProcessSeriesLikelihood(identity, t, d, sigma,
                                           kernel=kernel,
                                           normalised=normalised)


@functools.lru_cache(maxsize=8)
def problem(p, n, kernel):
    """t, data, sigma, n model rows and their hyper-parameters, deterministic
    from the arguments: t sorted uniform on [0, 10] with one pair of equal
    neighbours (from P = 2 on), sigma uniform in [0.1, 1], m the data plus
    N(0, 0.5^2), a log-uniform in [1e-2, 1e2], l in 10^[-1.5, 1], s in
    [1e-4, 1e-1] and, for 'sho', q uniform in [0.51, 50].  Nobody writes to
    the result."""
    rng = np.random.default_rng([p, n, GPS_KERNELS.index(kernel)])
    t = np.sort(rng.uniform(0, 10, size=p))
    if p > 1:
        t[p // 2] = t[p // 2 - 1]
    sigma = rng.uniform(0.1, 1, size=p)
    d = rng.normal(size=p)
    m = d + 0.5 * rng.normal(size=(n, p))
    cols = [10.0**rng.uniform(-2, 2, size=n), 10.0**rng.uniform(-1.5, 1, size=n),
            10.0**rng.uniform(-4, -1, size=n)]
    if kernel == 'sho':
        cols.append(rng.uniform(0.51, 50, size=n))
    h = np.stack(cols, axis=1)
    for arr in (t, d, sigma, m, h):
        arr.setflags(write=False)
    return t, d, sigma, m, h


@functools.lru_cache(maxsize=8)
def truth(p, n, kernel):
    """The twin in ``np.longdouble`` on ``problem``: the recursion itself,
    from the same float64 steps, data, sigma^2 and model outputs."""
    t, d, sigma, m, h = problem(p, n, kernel)
    out = make(t, d, sigma, kernel).numpy_from_model(m, h, dtype=LD)
    assert out.dtype == LD and np.all(np.isfinite(out))
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=8)
def twin64(p, n, kernel):
    t, d, sigma, m, h = problem(p, n, kernel)
    out = make(t, d, sigma, kernel).numpy_from_model(m, h)
    assert out.dtype == np.float64 and np.all(np.isfinite(out))
    out.setflags(write=False)
    return out


def budget(got64, want):
    """The device's tolerance per row from a float64 twin and the long-double
    truth of the same case: eight times the twin's largest error -- three bits
    for the device's different roundings of exp and sincos, its reciprocal
    and its log of a product of mantissas -- and at least 64 eps |truth|."""
    err = float(np.max(np.abs(got64.astype(LD) - want)))
    return np.maximum(8.0 * err, 64 * EPS * np.abs(want.astype(float)))


def case_budget(p, n, kernel):
    return budget(twin64(p, n, kernel), truth(p, n, kernel))


# ------------------------------------------------------ against dense Cholesky

def cholesky_value(k, r):
    """-1/2 (r^T K^-1 r + log det K) of the (n, P, P) matrices ``k`` and the
    (n, P) residuals ``r`` by a column Cholesky in their own type."""
    k = k.copy()
    n, p = r.shape
    y = r.copy()
    log_det = np.zeros(n, k.dtype)
    for j in range(p):
        piv = k[:, j, j]
        assert np.all(piv > 0)
        root = np.sqrt(piv)
        col = k[:, j:, j] / root[:, None]
        y[:, j] = y[:, j] / root
        y[:, j + 1:] -= col[:, 1:] * y[:, j, None]
        k[:, j + 1:, j + 1:] -= col[:, 1:, None] * col[:, None, 1:]
        log_det += 2 * np.log(root)
    return -(np.sum(y * y, axis=1) + log_det) / 2


def correlation(kernel, r, q):
    if kernel == 'sho':
        return sho_correlation(r, q)
    return gp_correlation(kernel, r)


def dense_truth(like, m, h):
    """Long-double dense evaluation of the defining K.  The times are the
    running sums of the float64 steps the filter reads, exact in long
    double."""
    tt = np.cumsum(like._dt.astype(LD))
    dist = np.abs(tt[:, None] - tt[None, :])
    a, l, s = (h[:, i].astype(LD)[:, None, None] for i in range(3))
    q = h[:, 3].astype(LD)[:, None, None] if like.kernel == 'sho' else None
    k = a * correlation(like.kernel, dist * (1 / l), q)
    k += np.eye(len(tt), dtype=LD) * (like._sigma2.astype(LD) + s)
    return cholesky_value(k, m.astype(LD) - like.data.astype(LD))


def dense_float64(like, t, d, sigma, m, h):
    """The dense class's numpy path (LAPACK) on the same inputs."""
    if like.kernel != 'sho':
        dense = GaussianProcessLikelihood(identity, t, d, sigma,
                                          kernel=like.kernel, cov='hyper',
                                          normalised=False)
        return dense.numpy_from_model(m, h)
    dense = GaussianProcessLikelihood(identity, t, d, sigma, cov='full',
                                      normalised=False)
    a, l, s, q = (h[:, i, None, None] for i in range(4))
    c = a * sho_correlation(dense.dist / l, q) + s * np.eye(len(t))
    return dense.numpy_from_model(m, c)


@pytest.mark.parametrize('kernel', GPS_KERNELS)
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
    print('P = %d, %s: long-double twin - dense Cholesky %.2g relative; '
          'float64 twin error %.3g, dense LAPACK error %.3g, ratio %.3g' % (
              p, kernel, rel, err, err_dense, err / err_dense))
    assert rel <= 1e-14
    assert err <= 4 * err_dense


def test_sho_near_critical_damping_is_matern32():
    """q -> 1/2: rho -> (1 + r) exp(-r), Matern-3/2 at l / sqrt(3)."""
    r = np.linspace(0, 30, 301).astype(LD)
    got = sho_correlation(r, LD(0.5) + LD(1e-9))
    want = gp_correlation('matern32', r / np.sqrt(LD(3)))
    assert np.max(np.abs(got - want)) < 1e-7


# ------------------------------------------------------------------ its limits

def test_white_noise_is_a_sum_of_normal_log_densities():
    for kernel in GPS_KERNELS:
        t, d, sigma, m, h = problem(40, 9, kernel)
        h = h.copy()
        h[:, 0] = 0.0
        like = make(t, d, sigma, kernel, normalised=True)
        got = like.numpy_from_model(m, h)
        v = sigma**2 + h[:, 2:3]
        want = -0.5 * np.sum((m - d)**2 / v + np.log(2 * np.pi * v), axis=1)
        assert np.allclose(got, want, rtol=1e-13, atol=0)
        noise = GaussianNoiseLikelihood(identity, d, sigma, noise='full')
        other = noise.numpy_from_model(m, np.broadcast_to(h[:, 2:3], m.shape))
        assert np.allclose(got, other, rtol=1e-13, atol=0)


@pytest.mark.parametrize('kernel', GPS_KERNELS)
def test_a_gap_beyond_the_cap_decouples_the_halves(kernel):
    t, d, sigma, m, h = problem(30, 6, kernel)
    h = h.copy()
    if kernel == 'sho':
        h[:, 3] = np.linspace(0.6, 5.0, len(h))  # exp(-1e4 / (2 q)) is 0
    t = t.copy()
    t[17:] += 1.01 * GPS_CAP * h[:, 1].max()
    # in long double, where the order of the sums does not show
    whole = make(t, d, sigma, kernel).numpy_from_model(m, h, dtype=LD)
    left = make(t[:17], d[:17], sigma[:17], kernel).numpy_from_model(
        m[:, :17], h, dtype=LD)
    right = make(t[17:], d[17:], sigma[17:], kernel).numpy_from_model(
        m[:, 17:], h, dtype=LD)
    assert np.all(np.isfinite(whole))
    assert np.all(np.abs(whole - (left + right)) <=
                  1e-15 * (np.abs(left) + np.abs(right)))
    # an infinite dt / l is the same gap, not a NaN
    h[:, 1] = 1e-300
    t2 = np.r_[t[:17], t[17:] + 1e10]
    assert np.all(np.isfinite(make(t2, d, sigma, kernel).numpy_from_model(m, h)))


# ---------------------------------------------------------------- the NaN rules

BAD_HYPER = [(0, -1.0), (0, np.nan), (0, np.inf), (1, 0.0), (1, -2.0),
             (1, np.nan), (1, np.inf), (2, -1e-3), (2, np.nan), (2, np.inf)]
BAD_Q = [(3, 0.5), (3, 0.2), (3, -1.0), (3, np.nan), (3, np.inf)]


@pytest.mark.parametrize('kernel', GPS_KERNELS)
def test_nan_rules_of_the_twin(kernel):
    t, d, sigma, m, h = problem(20, 24, kernel)
    like = make(t, d, sigma, kernel)
    clean = like.numpy_from_model(m, h)
    assert np.all(np.isfinite(clean))
    m2, h2 = m.copy(), h.copy()
    bad = BAD_HYPER + (BAD_Q if kernel == 'sho' else [])
    rows = []
    for i, (col, value) in enumerate(bad):
        h2[i, col] = value
        rows.append(i)
    for i, value in zip((16, 17, 18), (np.nan, np.inf, -np.inf)):
        m2[i, (0, 7, 19)[i - 16]] = value
        rows.append(i)
    got = like.numpy_from_model(m2, h2)
    assert np.all(np.isnan(got[rows]))
    rest = np.setdiff1d(np.arange(24), rows)
    assert len(rest) > 0 and np.array_equal(got[rest], clean[rest])
    # a = 0 is white noise; sigma = s = 0 at a repeated time is a zero pivot
    h3 = h.copy()
    h3[:, 0] = 0.0
    assert np.all(np.isfinite(like.numpy_from_model(m, h3)))
    bare = make(t, d, None, kernel)
    h4 = h.copy()
    h4[::2, 2] = 0.0
    got = bare.numpy_from_model(m, h4)
    assert np.all(np.isnan(got[::2])) and np.all(np.isfinite(got[1::2]))


def test_constructor_refuses_bad_arguments():
    t = np.linspace(0, 1, 5)
    d = np.arange(5.0)
    GaussianProcessSeriesLikelihood(identity, t, d)
    GaussianProcessSeriesLikelihood(identity, np.zeros(5), d, np.zeros(5))
    with pytest.raises(ValueError, match='callable'):
        GaussianProcessSeriesLikelihood(None, t, d)
    with pytest.raises(ValueError, match='must not decrease'):
        GaussianProcessSeriesLikelihood(identity, t[::-1], d)
    with pytest.raises(ValueError, match='must not decrease'):
        GaussianProcessSeriesLikelihood(identity, np.r_[0, 2, 1, 3, 4.0], d)
    with pytest.raises(ValueError, match='no finite state'):
        GaussianProcessSeriesLikelihood(identity, t, d, kernel='sqexp')
    with pytest.raises(ValueError, match='kernel must be one of'):
        GaussianProcessSeriesLikelihood(identity, t, d, kernel='periodic')
    for bad_t in (t[:4], t.reshape(5, 1), np.r_[t[:4], np.nan],
                  np.r_[t[:4], np.inf]):
        with pytest.raises(ValueError, match='t must'):
            GaussianProcessSeriesLikelihood(identity, bad_t, d)
    with pytest.raises(ValueError, match='too spread out'):
        GaussianProcessSeriesLikelihood(identity,
                                        np.r_[-1.7e308, [1.7e308] * 4], d)
    with pytest.raises(ValueError, match='at least one'):
        GaussianProcessSeriesLikelihood(identity, np.zeros(0), np.zeros(0))
    with pytest.raises(ValueError, match='at most %d' % N_GPS_MAX):
        GaussianProcessSeriesLikelihood(identity, np.zeros(N_GPS_MAX + 1),
                                        np.zeros(N_GPS_MAX + 1))
    with pytest.raises(ValueError, match='vector'):
        GaussianProcessSeriesLikelihood(identity, t, d.reshape(5, 1))
    with pytest.raises(ValueError, match='data must be finite'):
        GaussianProcessSeriesLikelihood(identity, t, np.r_[d[:4], np.nan])
    for bad_sigma in (np.ones(4), -np.ones(5), np.r_[np.ones(4), np.nan]):
        with pytest.raises(ValueError, match='sigma'):
            GaussianProcessSeriesLikelihood(identity, t, d, bad_sigma)
    with pytest.raises(ValueError, match='too large'):
        GaussianProcessSeriesLikelihood(identity, t, d, np.full(5, 1e200))
    assert N_GPS_MAX == 1 << 20
    assert GPS_KERNELS == ('exp', 'matern32', 'matern52', 'sho')
    big = GaussianProcessSeriesLikelihood(identity, np.zeros(N_GPS_MAX),
                                          np.zeros(N_GPS_MAX))
    assert big.n_data == N_GPS_MAX and big.log_norm < 0


def test_model_outputs_are_checked():
    t, d, sigma, m, h = problem(6, 4, 'matern32')
    like = make(t, d, sigma, 'matern32')
    sho = make(t, d, sigma, 'sho')
    with pytest.raises(ValueError, match=r'shape \(n, 6\)'):
        like.numpy_from_model(m[:, :5], h)
    with pytest.raises(ValueError, match=r'shape \(4, 3\)'):
        like.numpy_from_model(m, h[:3])
    with pytest.raises(ValueError, match=r'shape \(4, 4\)'):
        sho.numpy_from_model(m, h)
    with pytest.raises(ValueError, match='both'):
        like.from_model(torch.from_numpy(m), h)
    with pytest.raises(ValueError, match='float64'):
        like.from_model(torch.from_numpy(m).float(), torch.from_numpy(h))
    with pytest.raises(ValueError, match='float64'):
        like.from_model(torch.from_numpy(m), torch.from_numpy(h).float())
    with pytest.raises(ValueError, match=r'shape \(4, 3\)'):
        like.from_model(torch.from_numpy(m), torch.from_numpy(h)[:, :2])
    with pytest.raises((TypeError, ValueError)):
        GaussianProcessSeriesLikelihood(lambda x: x, t, d).numpy(
            np.zeros((2, 6)))


def pair_model(x):
    return x[:, :6], x[:, 6:]


def test_pickle_round_trip_and_numpy_call():
    t, d, sigma, m, h = problem(6, 4, 'sho')
    like = GaussianProcessSeriesLikelihood(pair_model, t, d, sigma,
                                           kernel='sho')
    like._tables[0] = object()                   # stands for a device handle
    other = pickle.loads(pickle.dumps(like))
    assert other._tables == {} and like._tables
    assert other.kernel == 'sho' and other.n_data == 6
    x = np.concatenate([m, h], axis=1)
    want = like.numpy_from_model(m, h)
    assert np.array_equal(other.numpy(x), want)
    assert np.array_equal(like.numpy(x), want)
    assert like.log_norm == -0.5 * 6 * np.log(2 * np.pi)
    raw = make(t, d, sigma, 'sho')
    assert np.allclose(want, like.log_norm + raw.numpy_from_model(m, h),
                       rtol=4 * EPS, atol=0)


def test_exported_lazily():
    import nautilus_amd
    assert 'GaussianProcessSeriesLikelihood' in nautilus_amd._LAZY
    assert nautilus_amd.GaussianProcessSeriesLikelihood is \
        GaussianProcessSeriesLikelihood
    from nautilus_amd import likelihoods
    assert likelihoods.GP_KERNELS == ('sqexp', 'exp', 'matern32', 'matern52')


def test_constants_repeat_the_headers():
    import os
    import re
    from nautilus_amd import device
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    layout = open(os.path.join(root, 'nautilus_amd', 'csrc',
                               'nb_layout.h')).read()
    header = open(os.path.join(root, 'include', 'nautilus_hip.h')).read()
    assert int(re.search(r'#define NB_GPS_BLOCK (\d+)', layout).group(1)) == \
        device.GPS_BLOCK
    assert '#define NB_GPS_MAX_DATA (1 << 20)' in header
    assert device.GPS_MAX_DATA == N_GPS_MAX == 1 << 20
    for name, code in device.GPS_KERNELS.items():
        assert '#define NB_GPS_%s %d\n' % (name.upper(), code) in header
    assert tuple(device.GPS_KERNELS) == GPS_KERNELS
