"""Hyper-parameter sets of the emulator tests away from the defaults, and the
two references they are judged by: scikit-learn's ``MLPRegressor.fit`` and
the oracle's ``fit_network``.  Shared by test_emulator_hparams_cpu.py (oracle
against scikit-learn, exactly) and test_emulator_hparams_gpu.py (device
against both).

A and B move every constant of Adam and the stopping rule at once, C has no
first moment (beta_1 = 0: beta_1^t is 0 from the first step), D and E end at
``max_iter`` (E with tol = 0 and large betas, whose beta^t decay slowly).
The stop epochs of A on the 1000 x 5 fixture, 16 / 17 / 14 / 18 for seeds
0-3, straddle the 16 epochs of one launch of the device trainer."""

import functools
import warnings

import numpy as np

from conftest import load_golden

SETS = {
    'A': dict(learning_rate_init=3e-3, beta_1=0.8, beta_2=0.99, epsilon=1e-6,
              tol=1e-4, n_iter_no_change=3),
    'B': dict(learning_rate_init=2e-2, beta_1=0.5, beta_2=0.9, epsilon=1e-3,
              tol=1e-3, n_iter_no_change=1),
    'C': dict(learning_rate_init=1e-2, beta_1=0.0, beta_2=0.999, epsilon=1e-8,
              tol=1e-3, n_iter_no_change=1),
    'D': dict(max_iter=7),
    'E': dict(learning_rate_init=5e-3, beta_1=0.95, beta_2=0.9999, tol=0.0,
              n_iter_no_change=2, max_iter=12),
}

# stop epochs of the oracle on the standardised emulator_D5_E1, seeds 0-3
STOPS = {'A': [16, 17, 14, 18], 'B': [8, 6, 8, 8], 'C': [9, 7, 9, 9],
         'D': [7, 7, 7, 7], 'E': [12, 12, 12, 12]}

# the defaults of the reference (nautilus/neural.py:79-81)
DEFAULTS = dict(learning_rate_init=1e-2, beta_1=0.9, beta_2=0.999,
                epsilon=1e-8, tol=0.0, n_iter_no_change=10, max_iter=10000)


def oracle_kwargs(kw):
    """``fit_network`` arguments of MLPRegressor options."""
    names = dict(learning_rate_init='lr')
    return {names.get(k, k): v for k, v in kw.items()}


def device_hparams(kw):
    """``train_networks`` / ``train_ensembles`` hparams of MLPRegressor
    options (what ``emulator._hparams_from_kwargs`` returns)."""
    from nautilus_amd import emulator
    return emulator._hparams_from_kwargs(dict(kw))


@functools.lru_cache(maxsize=None)
def d5_data():
    """The standardised 1000 x 5 training set of emulator_D5_E1."""
    g = load_golden('emulator_D5_E1')
    x = (g['x'] - g['mean']) / g['scale']
    x.setflags(write=False)
    y = g['y']
    y.setflags(write=False)
    return x, y


def sklearn_fit(x, y, seed, kw):
    """``MLPRegressor.fit`` as the reference configures it (neural.py:79-83)
    with the options ``kw`` on top, BLAS on one thread (neural.py:10)."""
    from sklearn.neural_network import MLPRegressor
    from threadpoolctl import threadpool_limits
    opts = dict(hidden_layer_sizes=(100, 50, 20), alpha=0, random_state=seed,
                **{k: DEFAULTS[k] for k in ('learning_rate_init', 'tol',
                                            'n_iter_no_change', 'max_iter')})
    opts.update(kw)
    with threadpool_limits(limits=1), warnings.catch_warnings():
        warnings.simplefilter('ignore')        # ConvergenceWarning at max_iter
        return MLPRegressor(**opts).fit(x, y)


@functools.lru_cache(maxsize=None)
def d5_sklearn(name, seed, batch_size=None):
    """scikit-learn's fit of set ``name`` on ``d5_data``; computed once."""
    kw = dict(SETS[name])
    if batch_size is not None:
        kw['batch_size'] = batch_size
    return sklearn_fit(*d5_data(), seed, kw)


def stop_margin(loss_curve, kw):
    """How far the fit was from stopping at another epoch: the smallest
    |loss - (best - tol)| / loss over the epochs, the relative distance of
    the comparison ``loss > best - tol`` of the stopping rule
    (sklearn/_multilayer_perceptron.py:819-822) from flipping.  Infinite
    where ``max_iter`` ends the fit before the rule could fire whatever the
    losses are (set D: 7 epochs, patience 10)."""
    tol = kw.get('tol', DEFAULTS['tol'])
    patience = kw.get('n_iter_no_change', DEFAULTS['n_iter_no_change'])
    if kw.get('max_iter', DEFAULTS['max_iter']) <= patience:
        return np.inf
    best, margin = np.inf, np.inf
    for loss in loss_curve:
        if np.isfinite(best):
            margin = min(margin, abs(loss - (best - tol)) / loss)
        best = min(best, loss)
    return margin
