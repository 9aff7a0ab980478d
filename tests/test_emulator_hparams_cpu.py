"""Adam's constants and the stopping rule of ``neural_network_kwargs``
(``learning_rate_init``, ``beta_1``, ``beta_2``, ``epsilon``, ``tol``,
``n_iter_no_change``, ``max_iter``; the reference passes them to
MLPRegressor, neural.py:79-83).  CPU only.

a. The oracle's ``fit_network`` with these options IS scikit-learn's fit: bit
   for bit, so that the GPU tests (test_emulator_hparams_gpu.py) may use
   either as the judge.
b. Values scikit-learn rejects are rejected at ``Sampler.__init__``, and so
   is a ``max_iter`` beyond what the device trainer holds."""

import numpy as np
import pytest

import hparam_cases as hc
from nautilus_amd import emulator
from oracle import mlp_oracle as mo


@pytest.mark.parametrize('seed', [0, 1, 2, 3])
@pytest.mark.parametrize('name', sorted(hc.SETS))
def test_oracle_fit_equals_sklearn(name, seed):
    x, y = hc.d5_data()
    kw = hc.SETS[name]
    sk = hc.d5_sklearn(name, seed)
    ref = mo.fit_network(x, y, seed, **hc.oracle_kwargs(kw))
    assert ref.n_iter == sk.n_iter_ == hc.STOPS[name][seed]
    assert np.array_equal(ref.loss_curve, sk.loss_curve_)
    for k in range(4):
        assert np.array_equal(ref.coefs[k], sk.coefs_[k])
        assert np.array_equal(ref.intercepts[k], sk.intercepts_[k])


def test_oracle_emulator_takes_adam_constants():
    """``oracle.mlp_oracle.Emulator.train`` passes the three constants on
    (it used to raise on them)."""
    g = hc.load_golden('emulator_D5_E1')
    emu = mo.Emulator.train(g['x'], g['y'], n_networks=2,
                            neural_network_kwargs=hc.SETS['B'])
    xs = (g['x'] - emu.mean) / emu.scale
    for seed, net in enumerate(emu.networks):
        sk = hc.sklearn_fit(xs, g['y'], seed, hc.SETS['B'])
        assert net.n_iter == sk.n_iter_
        assert np.array_equal(net.loss_curve, sk.loss_curve_)
        assert np.array_equal(net.coefs[0], sk.coefs_[0])


def test_set_a_straddles_a_launch():
    """What set A is for: stops inside the first launch of the device
    trainer, exactly at its end and inside the second."""
    stops = hc.STOPS['A']
    c = emulator.EPOCH_CHUNK
    assert min(stops) < c and c in stops and max(stops) > c
    assert sum(s > c for s in stops) >= 2


BAD = [('learning_rate_init', 0), ('beta_1', 1.0), ('beta_1', -0.1),
       ('beta_2', 1.0), ('epsilon', 0), ('tol', -1e-3),
       ('n_iter_no_change', 0), ('max_iter', 0)]


@pytest.mark.parametrize('key,val', BAD)
def test_values_sklearn_rejects_are_refused_early(key, val):
    from sklearn.neural_network import MLPRegressor
    from nautilus_amd import GaussianLikelihood, Sampler, unit_prior
    rng = np.random.default_rng(0)
    with pytest.raises(ValueError):
        MLPRegressor(**{key: val}).fit(rng.random((20, 2)), rng.random(20))
    with pytest.raises(ValueError, match=key):
        emulator.check_network_kwargs({key: val})
    like = GaussianLikelihood([0.5, 0.5], 0.01 * np.eye(2))
    with pytest.raises(ValueError, match=key):
        Sampler(unit_prior, like, n_dim=2, n_live=100,
                neural_network_kwargs={key: val})
    # NeuralNetworkEmulator.train refuses it before touching the data
    with pytest.raises(ValueError, match=key):
        emulator.NeuralNetworkEmulator.train(
            np.zeros((10, 2)), np.zeros(10), neural_network_kwargs={key: val})


@pytest.mark.parametrize('key,val', [
    ('learning_rate_init', np.nan), ('beta_2', np.nan), ('epsilon', np.inf),
    ('tol', np.nan), ('tol', 'small'), ('beta_1', None),
    ('n_iter_no_change', 2.5), ('n_iter_no_change', True),
    ('max_iter', 100.0), ('max_iter', -5)])
def test_values_the_device_cannot_hold_are_refused(key, val):
    """NaN, non-numbers and non-integers where the C ABI takes an int32."""
    with pytest.raises(ValueError, match=key):
        emulator.check_network_kwargs({key: val})


def test_max_iter_beyond_the_device_limit():
    assert emulator.MAX_ITER == 10000
    with pytest.raises(ValueError, match='10000'):
        emulator.check_network_kwargs(dict(max_iter=10001))
    with pytest.raises(ValueError, match='10000'):
        emulator.check_network_kwargs(dict(max_iter=20000))


def test_boundary_values_pass():
    """The edges scikit-learn accepts."""
    from sklearn.neural_network import MLPRegressor
    for key, val in [('beta_1', 0.0), ('tol', 0.0), ('n_iter_no_change', 1),
                     ('max_iter', 10000)]:
        MLPRegressor(**{key: val})._validate_params()
        emulator.check_network_kwargs({key: val})
    hp = emulator._hparams_from_kwargs(dict(
        beta_1=0.0, tol=0.0, n_iter_no_change=np.int64(1), max_iter=10000,
        beta_2=0, epsilon=1e-300, learning_rate_init=5))
    assert hp == dict(beta1=0.0, tol=0.0, n_iter_no_change=1, max_iter=10000,
                      beta2=0.0, epsilon=1e-300, lr=5.0)
    # plain Python numbers for the C ABI
    assert type(hp['n_iter_no_change']) is int and type(hp['beta2']) is float


def test_header_limit_matches():
    """The limit the C ABI enforces (nb_trainer_set_hparams) is the one the
    host names."""
    import os
    import re
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(root, 'nautilus_amd', 'csrc',
                           'nb_mlp_train.hip')) as f:
        m = re.search(r'max_iter > (\d+)\)', f.read())
    assert m and int(m.group(1)) == emulator.MAX_ITER
