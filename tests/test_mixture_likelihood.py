"""Host side of ``GaussianMixtureLikelihood`` with covariances and weights:
constructor validation, the numpy twin against scipy, pickling.  (The device
kernel is tested in test_mixture_likelihood_gpu.py.)"""

import pickle

import numpy as np
import pytest
from scipy.special import logsumexp
from scipy.stats import multivariate_normal

from nautilus_amd import GaussianLikelihood, GaussianMixtureLikelihood


def _problem(d, k, seed):
    rng = np.random.default_rng(seed)
    means = 0.25 + 0.5 * rng.random((k, d))
    a = rng.normal(size=(k, d, d))
    covs = 1e-3 * (a @ a.transpose(0, 2, 1) + 0.1 * np.eye(d))
    w = rng.random(k) + 0.05
    x = np.vstack([means[rng.integers(k, size=300)] +
                   0.03 * rng.normal(size=(300, d)), rng.random((300, d))])
    return means, covs, w, x


def _terms(means, covs, w, x):
    w = np.asarray(w) / np.sum(w)
    return np.array([np.log(w[i]) + multivariate_normal(
        means[i], covs[i]).logpdf(x) for i in range(len(means))])


@pytest.mark.parametrize('d, k', [(1, 2), (3, 5), (20, 4)])
def test_numpy_twin_matches_scipy(d, k):
    means, covs, w, x = _problem(d, k, 10 * d + k)
    like = GaussianMixtureLikelihood(means, covs=covs, weights=w)
    terms = _terms(means, covs, w, x)
    assert np.allclose(like.numpy(x), logsumexp(terms, axis=0), rtol=1e-11,
                       atol=1e-8)
    out, lab = like.numpy(x, labels=True)
    assert np.array_equal(out, like.numpy(x))
    assert lab.dtype == np.int32
    assert np.array_equal(lab, np.argmax(terms, axis=0))


def test_shared_covariance_and_default_weights():
    means, covs, _, x = _problem(4, 3, 1)
    like = GaussianMixtureLikelihood(means, covs=covs[0])
    assert like.covs.shape == (3, 4, 4)
    assert np.allclose(like.weights, 1 / 3)
    want = logsumexp(_terms(means, covs[[0, 0, 0]], np.ones(3), x), axis=0)
    assert np.allclose(like.numpy(x), want, rtol=1e-11, atol=1e-8)


def test_sigma_with_weights_is_isotropic():
    means, _, w, x = _problem(3, 4, 2)
    like = GaussianMixtureLikelihood(means, 0.05, weights=w)
    assert like.fused and like.parts is None and like.sigma == 0.05
    covs = np.broadcast_to(0.05**2 * np.eye(3), (4, 3, 3))
    assert np.allclose(like.covs, covs)
    want = logsumexp(_terms(means, covs, w, x), axis=0)
    assert np.allclose(like.numpy(x), want, rtol=1e-11, atol=1e-8)


def test_one_component_is_a_gaussian():
    means, covs, _, x = _problem(6, 1, 3)
    like = GaussianMixtureLikelihood(means, covs=covs)
    want = GaussianLikelihood(means[0], covs[0]).numpy(x)
    assert np.allclose(like.numpy(x), want, rtol=1e-11, atol=1e-8)
    assert np.all(like.numpy(x, labels=True)[1] == 0)


def test_attributes_of_both_constructors():
    means, covs, w, x = _problem(5, 3, 4)
    legacy = GaussianMixtureLikelihood(means, 0.03)
    assert not legacy.fused and legacy.sigma == 0.03
    assert len(legacy.parts) == 3
    assert all(isinstance(p, GaussianLikelihood) for p in legacy.parts)
    want = logsumexp([p.numpy(x) for p in legacy.parts], axis=0) - np.log(3)
    assert np.array_equal(legacy.numpy(x), want)
    like = GaussianMixtureLikelihood(means, covs=covs, weights=w, labels=True)
    assert like.fused and like.labels and like.device is True
    assert like.n_dim == 5 and like.n_components == 3
    assert like.means.shape == (3, 5) and like.covs.shape == (3, 5, 5)
    assert np.isclose(like.weights.sum(), 1.0)
    assert np.allclose(like.weights, w / w.sum())


def test_constructor_validation():
    means, covs, w, _ = _problem(3, 3, 5)
    new = GaussianMixtureLikelihood
    with pytest.raises(ValueError):
        new(means)                                        # neither
    with pytest.raises(ValueError):
        new(means, 0.1, covs=covs)                        # both
    with pytest.raises(ValueError):
        new(means, covs=covs[:2])                         # wrong K
    with pytest.raises(ValueError):
        new(means, covs=np.eye(4))                        # wrong D
    bad = covs.copy()
    bad[1] = -bad[1]
    with pytest.raises(ValueError, match='component 1'):
        new(means, covs=bad)
    bad = covs.copy()
    bad[2, 0, 0] = np.nan
    with pytest.raises(ValueError, match='component 2'):
        new(means, covs=bad)
    for weights in ([1.0, 2.0], [1.0, 0.0, 1.0], [1.0, -1.0, 1.0],
                    [1.0, np.inf, 1.0], [1.0, np.nan, 1.0]):
        with pytest.raises(ValueError):
            new(means, covs=covs, weights=weights)
    for sigma in (0.0, -1.0, np.inf):
        with pytest.raises(ValueError):
            new(means, sigma, weights=w)
    with pytest.raises(ValueError):
        new(means * np.nan, covs=covs)


def test_pickle_round_trip():
    means, covs, w, x = _problem(4, 3, 6)
    like = GaussianMixtureLikelihood(means, covs=covs, weights=w, labels=True)
    like._tables['stand-in for a device handle'] = object()
    back = pickle.loads(pickle.dumps(like))
    assert back._tables == {}
    assert back.labels and back.fused
    out, lab = back.numpy(x, labels=True)
    want, want_lab = like.numpy(x, labels=True)
    assert np.array_equal(out, want) and np.array_equal(lab, want_lab)
    legacy = pickle.loads(pickle.dumps(GaussianMixtureLikelihood(means, 0.1)))
    assert legacy.sigma == 0.1 and len(legacy.parts) == 3
