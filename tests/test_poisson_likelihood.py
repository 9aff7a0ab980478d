"""Host side of ``PoissonDataLikelihood``: the numpy twin against mpmath and
scipy, the constant, the edge-case rules, constructor validation, pickling
and the ABI entries.  (The device kernel is tested in
test_poisson_likelihood_gpu.py.)"""

import os
import pickle

import numpy as np
import pytest
import torch

from nautilus_amd import PoissonDataLikelihood

EPS = 2.0**-52
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def identity(x):
    return x


def _exact(mu, k):
    """D(mu, k) and B = |mu - k| + k |log(mu / k)| (B = mu for k = 0) from
    the doubles themselves at 60 digits."""
    import mpmath as mp
    d, b = [], []
    with mp.workdps(60):
        for m_, k_ in zip(mu, k):
            m_, k_ = mp.mpf(float(m_)), mp.mpf(float(k_))
            if k_ == 0:
                d.append(m_)
                b.append(m_)
            else:
                lg = mp.log(m_ / k_)
                d.append(m_ - k_ - k_ * lg)
                b.append(abs(m_ - k_) + k_ * abs(lg))
    return d, b


def test_twin_matches_mpmath_and_the_naive_form_does_not():
    """Per element |D_twin - D_true| <= 4 eps B over counts from 0.3 to 1e7
    and model / data ratios from 1 +- 1e-6 to e^+-30; the form k log mu - mu
    (against k log k - k) misses the same bound on the same inputs, so the
    inputs do exercise the cancellation."""
    import mpmath as mp
    from scipy.special import xlogy
    rng = np.random.default_rng(2026)
    worst = worst_naive = 0.0
    for lam in (0.3, 3, 30, 1e3, 1e5, 1e7):
        for spread in (1e-6, 1e-3, 0.1, 1, 10):
            k = rng.poisson(lam, size=64).astype(float)
            mu = lam * np.exp(spread * rng.normal(size=64))
            like = PoissonDataLikelihood(identity, k)
            twin = like.numpy_deviance(mu[None])[0]
            assert np.all(twin >= 0.0)
            naive = (xlogy(k, k) - k) - (xlogy(k, mu) - mu)
            d, b = _exact(mu, k)
            for j in range(64):
                unit = EPS * float(b[j])
                if unit == 0.0:                  # mu == k exactly
                    assert twin[j] == 0.0
                    continue
                worst = max(worst, float(abs(mp.mpf(twin[j]) - d[j])) / unit)
                worst_naive = max(worst_naive,
                                  float(abs(mp.mpf(naive[j]) - d[j])) / unit)
    print('largest error in eps B: twin %.3g, k log mu - mu %.3g' % (
        worst, worst_naive))
    assert worst <= 4.0
    assert worst_naive > 4.0


@pytest.mark.parametrize('lam', [0.5, 5.0, 50.0])
def test_normalised_matches_scipy(lam):
    from scipy.special import gammaln
    from scipy.stats import poisson
    rng = np.random.default_rng(int(10 * lam))
    p, n = 64, 20
    k = np.minimum(rng.poisson(lam, size=p), 100).astype(float)
    e = 0.5 + rng.random(p)
    b = 0.1 * lam * rng.random(p)
    m = lam * np.exp(0.3 * rng.normal(size=(n, p)))
    like = PoissonDataLikelihood(identity, k, exposure=e, background=b)
    mu = e * m + b
    want = poisson.logpmf(k, mu).sum(1)
    tol = 8 * EPS * np.sum(k * np.abs(np.log(mu)) + mu + gammaln(k + 1),
                           axis=1)
    got = like.numpy_from_model(m)
    print('lambda = %g: largest error %.3g of the budget' % (
        lam, (np.abs(got - want) / tol).max()))
    assert np.all(np.abs(got - want) <= tol)
    assert np.array_equal(like.numpy(m), got)    # the identity model
    assert like.n_data == p and like.device is True
    # without the constant: -1/2 of the Cash statistic
    cash = 2 * np.sum(mu - k + k * (np.log(np.where(k > 0, k, 1.0)) -
                                    np.log(mu)), axis=1)
    raw = PoissonDataLikelihood(identity, k, exposure=e, background=b,
                                normalised=False)
    assert raw.log_const == 0.0
    assert np.allclose(raw.numpy_from_model(m), -0.5 * cash, rtol=1e-12)


def test_constant_matches_mpmath():
    import mpmath as mp
    from nautilus_amd.likelihoods import poisson_log_const
    ks = np.array([0, 0.5, 1, 15, 16, 17, 1e3, 1e7])
    got = poisson_log_const(ks)
    with mp.workdps(60):
        for k, g in zip(ks, got):
            if k == 0:
                assert g == 0.0
                continue
            km = mp.mpf(float(k))
            true = km * mp.log(km) - km - mp.loggamma(km + 1)
            err = float(abs(mp.mpf(float(g)) - true))
            bound = 4 * EPS * max(1.0, abs(float(true)))
            print('k = %g: C = %.17g, error %.3g of the bound' % (
                k, g, err / bound))
            assert err <= bound
    like = PoissonDataLikelihood(identity, ks)
    assert like.log_const == float(np.sum(got))


def test_edge_cases_through_the_twin():
    rng = np.random.default_rng(5)
    p, n = 17, 12
    k = rng.poisson(4.0, size=p).astype(float)
    k[3] = 0.0
    k[8] = 6.0
    m = 4.0 * np.exp(0.2 * rng.normal(size=(n, p)))
    like = PoissonDataLikelihood(identity, k)
    clean = like.numpy_from_model(m)
    assert np.all(np.isfinite(clean))
    dirty = m.copy()
    dirty[1, 8] = 0.0                  # mu = 0, k > 0
    dirty[2, 3] = 0.0                  # mu = 0, k = 0
    dirty[4, 8] = -1e-300              # negative
    dirty[5, 0] = np.nan
    dirty[6, 16] = np.inf
    dirty[7, 8] = 0.0                  # -inf and NaN in one row
    dirty[7, 9] = np.nan
    dirty[9, 3] = -np.inf
    out = like.numpy_from_model(dirty)
    assert out[1] == -np.inf
    assert np.isfinite(out[2])
    assert out[2] == like.numpy_from_model(dirty[2:3])[0]
    for i in (4, 5, 6, 7, 9):
        assert np.isnan(out[i]), i
    keep = np.ones(n, bool)
    keep[[1, 2, 4, 5, 6, 7, 9]] = False
    assert np.array_equal(out[keep], clean[keep])
    # mu = 0, k = 0 contributes exactly 0: the row without that bin
    rest = np.delete(np.arange(p), 3)
    part = PoissonDataLikelihood(identity, k[rest], normalised=False)
    whole = PoissonDataLikelihood(identity, k, normalised=False)
    d = whole.numpy_deviance(dirty[2:3])
    assert d[0, 3] == 0.0
    assert np.array_equal(np.delete(d, 3, axis=1),
                          part.numpy_deviance(dirty[2:3, rest]))
    # the background alone keeps a bin alive
    bg = PoissonDataLikelihood(identity, k, background=np.full(p, 0.5))
    assert np.isfinite(bg.numpy_from_model(dirty[1:2])[0])


def test_constructor_validation():
    new = PoissonDataLikelihood
    k = np.array([0.0, 1.0, 2.5, 7.0])
    assert new(identity, k).n_data == 4
    with pytest.raises(ValueError):
        new(None, k)                                          # no model
    for bad in ([], k.reshape(2, 2), np.r_[k[:3], np.nan],
                np.r_[k[:3], np.inf], np.r_[k[:3], -1.0]):
        with pytest.raises(ValueError):
            new(identity, bad)
    with pytest.raises(ValueError):
        new(identity, k, exposure=np.ones(3))                 # wrong shape
    with pytest.raises(ValueError):
        new(identity, k, exposure=2.0)
    for e in (0.0, -1.0, np.inf, np.nan):
        with pytest.raises(ValueError):
            new(identity, k, exposure=np.r_[1.0, 1.0, 1.0, e])
    with pytest.raises(ValueError):
        new(identity, k, background=np.zeros(5))              # wrong shape
    for b in (-1e-3, np.inf, np.nan):
        with pytest.raises(ValueError):
            new(identity, k, background=np.r_[0.0, 0.0, 0.0, b])
    assert new(identity, k, background=np.zeros(4)).n_data == 4
    # a positive count whose reciprocal overflows
    for tiny in (5e-324, 1e-310):
        with pytest.raises(ValueError, match='too small'):
            new(identity, np.r_[k[:3], tiny])
    assert new(identity, np.r_[k[:3], 1e-300]).n_data == 4
    # 2^20 bins is the largest supported
    assert new(identity, np.zeros(1 << 20)).n_data == 1 << 20
    with pytest.raises(ValueError, match=str(1 << 20)):
        new(identity, np.zeros((1 << 20) + 1))


def test_model_output_validation():
    k = np.array([0.0, 1.0, 2.5, 7.0])
    m = np.full((5, 4), 2.0)
    like = PoissonDataLikelihood(identity, k)
    with pytest.raises(ValueError):
        like.numpy_from_model(m[:, :3])
    with pytest.raises(ValueError):
        like.numpy_from_model(m[0])
    # the device entry checks before it touches the GPU
    with pytest.raises(ValueError):
        like.from_model(torch.from_numpy(m[:, :3]))
    with pytest.raises(ValueError):
        like.from_model(torch.from_numpy(m[0]))
    with pytest.raises(ValueError):
        like.from_model(torch.from_numpy(m).float())
    with pytest.raises(ValueError):
        like.from_model(m.astype(np.float32))


def test_numpy_twin_runs_the_model_on_the_cpu():
    rng = np.random.default_rng(2)
    a = torch.from_numpy(rng.random((7, 3)) + 0.1)
    k = rng.poisson(3.0, size=7).astype(float)
    seen = []

    def model(x):
        seen.append(x)
        return x @ a.T

    like = PoissonDataLikelihood(model, k)
    x = rng.random((11, 3)) + 0.5
    m = (torch.from_numpy(x) @ a.T).numpy()
    assert np.array_equal(like.numpy(x), like.numpy_from_model(m))
    assert isinstance(seen[0], torch.Tensor) and not seen[0].is_cuda
    assert seen[0].dtype == torch.float64


def test_pickle_round_trip():
    rng = np.random.default_rng(8)
    k = rng.poisson(9.0, size=6).astype(float)
    m = 9.0 + rng.random((5, 6))
    like = PoissonDataLikelihood(identity, k, exposure=np.full(6, 2.0),
                                 background=np.full(6, 0.25))
    like._tables['stand-in for a device handle'] = object()
    back = pickle.loads(pickle.dumps(like))
    assert back._tables == {}
    assert back.n_data == 6 and back.log_const == like.log_const
    assert np.array_equal(back.numpy_from_model(m), like.numpy_from_model(m))


def test_abi_entries():
    from nautilus_amd import _lib
    header = open(os.path.join(ROOT, 'include', 'nautilus_hip.h')).read()
    for name in ('nb_poisson_create', 'nb_poisson_loglike',
                 'nb_poisson_destroy'):
        assert name in _lib._SIGNATURES
        assert 'int %s(' % name in header
    assert '#define NB_POISSON_MAX_DATA (1 << 20)' in header
