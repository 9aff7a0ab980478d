"""Host side of ``GaussianDataLikelihood``: constructor validation, the numpy
twin against scipy, pickling.  (The device kernel is tested in
test_data_likelihood_gpu.py.)"""

import pickle

import numpy as np
import pytest
import torch
from scipy.stats import multivariate_normal, norm

from nautilus_amd import GaussianDataLikelihood

RTOL, ATOL = 1e-11, 1e-8          # the band tests/test_hip_parity.py holds the
#                                   likelihoods to


def identity(x):
    return x


def _problem(p, seed, n=40):
    """C = 1e-2 (A A^T / P + 0.5 I), model rows d + 0.3 sqrt(diag C) N(0, 1)."""
    rng = np.random.default_rng(seed)
    a = rng.normal(size=(p, p))
    cov = 1e-2 * (a @ a.T / p + 0.5 * np.eye(p))
    d = rng.normal(size=p)
    m = d + 0.3 * np.sqrt(np.diag(cov)) * rng.normal(size=(n, p))
    return d, cov, m


@pytest.mark.parametrize('p', [1, 3, 17, 129, 257])
def test_numpy_twin_matches_scipy(p):
    d, cov, m = _problem(p, p)
    like = GaussianDataLikelihood(identity, d, cov=cov)
    want = np.atleast_1d(multivariate_normal(d, cov).logpdf(m))
    got = like.numpy_from_model(m)
    err = np.abs(got - want) / (ATOL + RTOL * np.abs(want))
    print('P = %d: largest error %.3g of the band' % (p, err.max()))
    assert np.allclose(got, want, rtol=RTOL, atol=ATOL)
    # numpy(x) runs the model on the CPU: the identity model of P parameters
    assert np.array_equal(like.numpy(m), got)
    assert like.n_data == p and like.device is True
    assert np.array_equal(like.data, d) and np.array_equal(like.cov, cov)
    assert like.sigma is None
    sign, log_det = np.linalg.slogdet(cov)
    assert np.isclose(like.log_norm,
                      -0.5 * (p * np.log(2 * np.pi) + log_det), rtol=1e-12)


@pytest.mark.parametrize('p', [1, 3, 17, 129, 257])
def test_sigma_matches_scipy(p):
    d, cov, m = _problem(p, 50 + p)
    sigma = np.sqrt(np.diag(cov))
    like = GaussianDataLikelihood(identity, d, sigma=sigma)
    want = np.sum(norm.logpdf(m, loc=d, scale=sigma), axis=1)
    assert np.allclose(like.numpy_from_model(m), want, rtol=RTOL, atol=ATOL)
    assert like.cov is None and np.array_equal(like.sigma, sigma)
    # a diagonal cov is the same likelihood
    full = GaussianDataLikelihood(identity, d, cov=np.diag(sigma**2))
    assert np.allclose(full.numpy_from_model(m), want, rtol=RTOL, atol=ATOL)


def test_unnormalised_has_no_constant():
    d, cov, m = _problem(5, 1)
    like = GaussianDataLikelihood(identity, d, cov=cov, normalised=False)
    assert like.log_norm == 0.0
    full = GaussianDataLikelihood(identity, d, cov=cov)
    assert np.allclose(like.numpy_from_model(m),
                       full.numpy_from_model(m) - full.log_norm,
                       rtol=RTOL, atol=ATOL)
    diag = GaussianDataLikelihood(identity, d, sigma=np.ones(5),
                                  normalised=False)
    assert diag.log_norm == 0.0
    assert np.allclose(diag.numpy_from_model(m),
                       -0.5 * np.sum((m - d)**2, axis=1), rtol=RTOL, atol=ATOL)


def test_numpy_twin_runs_the_model_on_the_cpu():
    rng = np.random.default_rng(2)
    a = torch.from_numpy(rng.normal(size=(7, 3)))
    d, cov, _ = _problem(7, 3)
    seen = []

    def model(x):
        seen.append(x)
        return x @ a.T

    like = GaussianDataLikelihood(model, d, cov=cov)
    x = rng.random((11, 3))
    want = np.atleast_1d(multivariate_normal(d, cov).logpdf(x @ a.numpy().T))
    assert np.allclose(like.numpy(x), want, rtol=RTOL, atol=ATOL)
    assert isinstance(seen[0], torch.Tensor) and not seen[0].is_cuda
    assert seen[0].dtype == torch.float64


def test_non_finite_model_rows_are_nan():
    d, cov, m = _problem(17, 4)
    for kw in (dict(cov=cov), dict(sigma=np.sqrt(np.diag(cov)))):
        like = GaussianDataLikelihood(identity, d, **kw)
        clean = like.numpy_from_model(m)
        dirty = m.copy()
        dirty[5, 3] = np.nan
        dirty[19, 16] = np.inf
        out = like.numpy_from_model(dirty)
        assert np.isnan(out[5]) and np.isnan(out[19])
        keep = np.ones(len(m), bool)
        keep[[5, 19]] = False
        assert np.array_equal(out[keep], clean[keep])


def test_constructor_validation():
    d, cov, _ = _problem(4, 5)
    sigma = np.sqrt(np.diag(cov))
    new = GaussianDataLikelihood
    with pytest.raises(ValueError):
        new(identity, d)                                      # neither
    with pytest.raises(ValueError):
        new(identity, d, cov=cov, sigma=sigma)                # both
    with pytest.raises(ValueError):
        new(None, d, cov=cov)                                 # no model
    for bad_data in (d * np.nan, np.r_[d[:3], np.inf], [], d.reshape(2, 2)):
        with pytest.raises(ValueError):
            new(identity, bad_data, sigma=np.ones(np.size(bad_data)))
    with pytest.raises(ValueError):
        new(identity, d, cov=cov[:3, :3])                     # wrong shape
    with pytest.raises(ValueError):
        new(identity, d, cov=cov[0])
    with pytest.raises(ValueError):
        new(identity, d, sigma=sigma[:3])
    with pytest.raises(ValueError):
        new(identity, d, sigma=0.1)
    q, _ = np.linalg.qr(np.random.default_rng(6).normal(size=(4, 4)))
    negative = (q * np.array([1.0, 0.5, 0.2, -0.1])) @ q.T   # one eigenvalue < 0
    nan = cov.copy()
    nan[1, 1] = np.nan
    lopsided = cov.copy()
    lopsided[0, 3] += 1e-3
    for bad in (negative, -cov, nan, lopsided, np.zeros((4, 4))):
        with pytest.raises(ValueError, match='cov is not positive definite'):
            new(identity, d, cov=bad)
    for s in (0.0, -1.0, np.inf, np.nan):
        with pytest.raises(ValueError):
            new(identity, d, sigma=np.r_[sigma[:3], s])
    # P = 4096 is the largest supported
    assert new(identity, np.zeros(4096), sigma=np.ones(4096)).n_data == 4096
    with pytest.raises(ValueError, match='4096'):
        new(identity, np.zeros(4097), sigma=np.ones(4097))


def test_model_output_validation():
    d, cov, m = _problem(4, 7)
    like = GaussianDataLikelihood(identity, d, cov=cov)
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


def test_pickle_round_trip():
    d, cov, m = _problem(6, 8)
    for kw in (dict(cov=cov), dict(sigma=np.sqrt(np.diag(cov)))):
        like = GaussianDataLikelihood(identity, d, **kw)
        like._tables['stand-in for a device handle'] = object()
        back = pickle.loads(pickle.dumps(like))
        assert back._tables == {}
        assert back.n_data == 6 and back.log_norm == like.log_norm
        assert np.array_equal(back.numpy_from_model(m),
                              like.numpy_from_model(m))
