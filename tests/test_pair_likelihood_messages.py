"""The four likelihoods whose model returns a pair -- noise, outlier, Gaussian
process and Gaussian-process series -- share how they take ``data`` and
``sigma`` and how ``from_model`` checks its two inputs (no GPU): every message
word for word, the order in which the errors come, and the attributes that
pickles and checkpoints hold."""

import pickle

import numpy as np
import pytest
import torch

from nautilus_amd.likelihoods import (
    N_GP_MAX, N_GPS_MAX, N_NOISE_MAX, GaussianNoiseLikelihood,
    GaussianOutlierLikelihood, GaussianProcessLikelihood,
    GaussianProcessSeriesLikelihood)


def identity(x):
    return x, x


# class, its limit on P, what it calls its second input, that input's width
CASES = {
    'noise': (GaussianNoiseLikelihood, N_NOISE_MAX, 'noise', 3),
    'outlier': (GaussianOutlierLikelihood, N_NOISE_MAX, 'mixture', 6),
    'gp': (GaussianProcessLikelihood, N_GP_MAX, 'covariance input', 3),
    'gps': (GaussianProcessSeriesLikelihood, N_GPS_MAX, 'hyper-parameters',
            3),
}


def make(name, data, sigma=None, model=identity, **kwargs):
    cls = CASES[name][0]
    t = kwargs.pop('t', np.arange(float(np.size(data))))
    if name in ('gp', 'gps'):
        return cls(model, t, data, sigma, **kwargs)
    return cls(model, data, sigma, **kwargs)


def message(fn, *args, **kwargs):
    with pytest.raises(ValueError) as err:
        fn(*args, **kwargs)
    return str(err.value)


@pytest.mark.parametrize('name', CASES)
def test_constructor_messages(name):
    n_max = CASES[name][1]
    d = np.r_[0.5, -1.0, 2.0, 0.0, 3.0]
    assert message(make, name, d, model=None) == 'model must be callable'
    for bad in (np.zeros(0), np.zeros((5, 1)), 1.0):
        assert message(make, name, bad, t=np.arange(5.0)) == \
            'data must be a vector of at least one number'
    assert message(make, name, np.zeros(n_max + 1)) == \
        'at most %d data points are supported, not %d' % (n_max, n_max + 1)
    for bad in (np.r_[d[:4], np.nan], np.r_[np.inf, d[1:]]):
        assert message(make, name, bad) == 'data must be finite'
    for bad in (np.ones(4), np.ones((5, 1)), -np.ones(5),
                np.r_[np.ones(4), np.nan], np.r_[np.inf, np.ones(4)]):
        assert message(make, name, d, bad) == \
            'sigma must be 5 finite numbers that are not negative'
    assert message(make, name, d, np.r_[np.ones(4), 1e200]) == \
        'sigma is too large: sigma^2 is not finite'


@pytest.mark.parametrize('name', CASES)
def test_constructor_error_order(name):
    """model, then the class's own options, then data, then t, then sigma."""
    d = np.r_[0.5, -1.0, 2.0]
    bad_d, bad_s = np.r_[0.5, np.nan, 2.0], -np.ones(3)
    assert message(make, name, bad_d, bad_s, model=None) == \
        'model must be callable'
    assert message(make, name, bad_d, bad_s) == 'data must be finite'
    assert message(make, name, np.zeros(0), bad_s) == \
        'data must be a vector of at least one number'
    if name == 'noise':
        assert message(make, name, bad_d, bad_s, noise='column') == \
            "noise must be 'row' or 'full', not 'column'"
    if name == 'gp':
        assert message(make, name, bad_d, bad_s, cov='diag',
                       kernel='periodic') == \
            "cov must be 'hyper' or 'full', not 'diag'"
        assert message(make, name, bad_d, bad_s, kernel='periodic') == \
            "kernel must be one of 'sqexp', 'exp', 'matern32', " \
            "'matern52', not 'periodic'"
        assert message(make, name, bad_d, bad_s, t=None) == \
            'data must be finite'
        assert message(make, name, d, bad_s, t=None) == \
            "cov='hyper' needs the input locations t"
        assert message(make, name, d, bad_s, t=np.zeros(2)) == \
            't must have shape (3,) or (3, d), not (2,)'
        assert message(make, name, d, bad_s, t=np.r_[0, np.nan, 1]) == \
            't must be finite'
        assert message(make, name, d, bad_s,
                       t=np.r_[-1.7e308, 0, 1.7e308]) == \
            't is too spread out: a distance is not finite'
    if name == 'gps':
        assert message(make, name, bad_d, bad_s, kernel='periodic') == \
            "kernel must be one of 'exp', 'matern32', 'matern52', 'sho', " \
            "not 'periodic'"
        assert message(make, name, d, bad_s, t=np.zeros(2)) == \
            't must have shape (3,), not (2,)'
        assert message(make, name, d, bad_s, t=np.r_[0, np.nan, 1]) == \
            't must be finite'
        assert message(make, name, d, bad_s, t=np.r_[0, 2.0, 1]) == \
            "t must not decrease (it is not sorted here: the model's " \
            'columns follow t)'
        assert message(make, name, d, bad_s,
                       t=np.r_[-1.7e308, 1.7e308, 1.7e308]) == \
            't is too spread out: a step is not finite'
    assert message(make, name, d, bad_s) == \
        'sigma must be 3 finite numbers that are not negative'


@pytest.mark.parametrize('name', CASES)
def test_constructor_attributes(name):
    d = np.r_[0.5, -1.0, 2.0]
    s = np.r_[0.0, 0.25, 1e-170]
    like = make(name, d, s)
    assert like.n_data == 3 and like._tables == {}
    assert np.array_equal(like.data, d) and like.data is not d
    assert np.array_equal(like.sigma, s) and like.sigma is not s
    assert np.array_equal(like._sigma2, s * s)
    assert like.log_norm == -0.5 * 3 * np.log(2 * np.pi)
    bare = make(name, d, normalised=False)
    assert bare.log_norm == 0.0
    for a in (bare.sigma, bare._sigma2):
        assert a.dtype == np.float64 and np.array_equal(a, np.zeros(3))
    # what a pickle holds, under these names
    like._tables[0] = object()
    state = pickle.loads(pickle.dumps(like)).__dict__
    assert state['_tables'] == {} and state['n_data'] == 3
    assert state['log_norm'] == like.log_norm
    for key in ('data', 'sigma', '_sigma2'):
        assert np.array_equal(state[key], getattr(like, key))


@pytest.mark.parametrize('name', CASES)
def test_from_model_messages(name):
    _, _, what, width = CASES[name]
    like = make(name, np.zeros(5))
    m, w = np.zeros((4, 5)), np.ones((4, width))
    both = 'the model output and the %s must both be torch tensors or ' \
        'both numpy arrays' % what
    assert message(like.from_model, torch.from_numpy(m), w) == both
    assert message(like.from_model, m, torch.from_numpy(w)) == both
    # kinds before types before shapes; the first output before the second
    assert message(like.from_model, torch.zeros(4, 4), w[:3]) == both
    f64 = 'the model output and the %s must be float64, not ' % what
    assert message(like.from_model, m[:, :4].astype(np.float32), w[:3]) == \
        f64 + 'float32'
    assert message(like.from_model, torch.from_numpy(m),
                   torch.ones(3, width)) == f64 + 'torch.float32'
    first = 'the model output must have shape (n, 5), not (4, 4)'
    second = 'the %s must have shape (4, %d), not ' % (what, width)
    for fn in (like.from_model, like.numpy_from_model):
        assert message(fn, m[:, :4], w[:3]) == first
        assert message(fn, m[0], w) == \
            'the model output must have shape (n, 5), not (5,)'
        assert message(fn, m, w[:3]) == second + '(3, %d)' % width
        assert message(fn, m, w[:, :2]) == second + '(4, 2)'
        assert message(fn, m, w[:, 0]) == second + '(4,)'
    assert message(like.from_model, torch.from_numpy(m),
                   torch.from_numpy(w)[:3]) == second + '(3, %d)' % width


def test_from_model_widths_of_the_other_modes():
    m = np.zeros((4, 5))
    full = make('noise', np.zeros(5), noise='full')
    assert message(full.from_model, m, np.ones((4, 3))) == \
        'the noise must have shape (4, 5), not (4, 3)'
    sho = make('gps', np.zeros(5), kernel='sho')
    assert message(sho.from_model, m, np.ones((4, 3))) == \
        'the hyper-parameters must have shape (4, 4), not (4, 3)'
    pair = make('gps', np.zeros(5), kernel=('exp', 'sho'))
    assert message(pair.from_model, m, np.ones((4, 3))) == \
        'the hyper-parameters must have shape (4, 6), not (4, 3)'
    gp = make('gp', np.zeros(5), cov='full')
    cov = 'the covariance input must have shape (4, 5, 5), not '
    assert message(gp.from_model, m, np.ones((4, 25))) == cov + '(4, 25)'
    # matrices of the right size arrive at the check as rows
    assert message(gp.from_model, m, np.ones((3, 5, 5))) == cov + '(3, 25)'
    assert message(gp.from_model, m, np.ones((4, 5, 4))) == cov + '(4, 5, 4)'
