"""Emulator training at minibatches above the reference's default of 200 rows
(``neural_network_kwargs=dict(batch_size=...)``, passed to MLPRegressor by
the reference, neural.py:79-83).  GPU only.

The trainer runs these on the LARGE instantiations of its kernels
(nb_mlp_train.hip): a stash laid out for the batch, FB workgroups that loop
over several row tiles, G jobs that contract every row tile of the minibatch.
Tolerances are those of the default batch's tests in test_hip_parity.py."""

import numpy as np
import pytest
import torch

from conftest import load_golden

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def dev():
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    from nautilus_amd import device
    return device


def _cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _close_to_oracle(net, ref, n_ep):
    assert net.n_iter_ == ref.n_iter == n_ep
    assert np.allclose(net.loss_curve_, ref.loss_curve, rtol=1e-9, atol=0)
    for k in range(4):
        assert np.allclose(net.coefs_[k], ref.coefs[k], rtol=0, atol=1e-8)
        assert np.allclose(net.intercepts_[k], ref.intercepts[k], rtol=0,
                           atol=1e-8)


@pytest.mark.parametrize('name', ['emulator_batch1000_D10_E2',
                                  'emulator_batch4096_D6_E2'])
def test_emulator_full_fit_at_large_batch_equals_sklearn(dev, name):
    """A WHOLE fit at batch 1000 (five minibatches per epoch) and 4096 (one
    full and one ragged minibatch) against scikit-learn's MLPRegressor.fit
    through the reference (make_golden_batch.py): equal stop epoch, loss
    curve, weights and predictions to rounding."""
    from nautilus_amd.emulator import NeuralNetworkEmulator
    g = load_golden(name)
    batch = int(g['batch_size'])
    emu = NeuralNetworkEmulator.train(
        g['x'], g['y'], n_networks=int(g['n_networks']),
        neural_network_kwargs=dict(batch_size=batch))
    assert np.allclose(emu.mean, g['mean'], rtol=1e-14, atol=1e-15)
    assert np.allclose(emu.scale, g['scale'], rtol=1e-13)
    for i, net in enumerate(emu.neural_networks):
        assert net.sk_params['batch_size'] == batch
        ref = g['loss_curve_%d' % i]
        assert net.n_iter_ == int(g['n_iter_%d' % i]) == len(ref)
        assert np.allclose(net.loss_curve_, ref, rtol=1e-9, atol=0)
        for k in range(4):
            assert np.allclose(net.coefs_[k], g['coef_%d_%d' % (i, k)],
                               rtol=0, atol=1e-10)
            assert np.allclose(net.intercepts_[k],
                               g['intercept_%d_%d' % (i, k)], rtol=0,
                               atol=1e-10)
    assert np.allclose(emu.predict(g['test']), g['predict'], rtol=0,
                       atol=1e-11)


@pytest.mark.parametrize('n', [700, 1001, 3000])
def test_large_batch_ragged_minibatches(dev, n):
    """batch 1000 with n < batch (one short minibatch per epoch),
    n = batch + 1 (a last minibatch of one row) and n a multiple of it."""
    from nautilus_amd import emulator
    from oracle import mlp_oracle as mo
    rng = np.random.default_rng(n)
    x = rng.normal(size=(n, 8))
    y = rng.random(n)
    nets, _ = emulator.train_networks(_cuda(x), _cuda(y), [0, 1],
                                      hparams=dict(batch=1000), max_epochs=3)
    for seed, net in zip([0, 1], nets):
        _close_to_oracle(net, mo.fit_network(x, y, seed, max_iter=3,
                                             batch_size=1000), 3)


@pytest.mark.parametrize('d', [64, 100, 128])
def test_large_batch_wide_inputs(dev, d):
    """Four to nine k-tiles in layer 1 (other job lists of G) at batch
    2000 with a ragged last minibatch."""
    from nautilus_amd import emulator
    from oracle import mlp_oracle as mo
    rng = np.random.default_rng(200 + d)
    n = 2500
    x = rng.normal(size=(n, d))
    y = rng.random(n)
    nets, _ = emulator.train_networks(_cuda(x), _cuda(y), [0, 3],
                                      hparams=dict(batch=2000), max_epochs=2)
    for seed, net in zip([0, 3], nets):
        _close_to_oracle(net, mo.fit_network(x, y, seed, max_iter=2,
                                             batch_size=2000), 2)


def test_large_batch_fleet_and_two_launch_fallback(dev, monkeypatch):
    """Two ensembles with different n (one above the batch, one below it)
    in one fleet trainer at batch 1024 against the oracle; with the resident
    kernel switched off (NB_TRAIN_NO_RESIDENT: a trainer per ensemble, two
    launches per step) the networks are the same."""
    from nautilus_amd import emulator
    from oracle import mlp_oracle as mo
    rng = np.random.default_rng(12)
    jobs, sets = [], []
    for n in (2300, 900):
        x = rng.normal(size=(n, 6))
        y = rng.random(n)
        sets.append((x, y))
        jobs.append(dict(xs=_cuda(x), y=_cuda(y), seeds=[0, 1],
                         hparams=dict(batch=1024), max_epochs=3))
    fleet = emulator.train_ensembles([dict(j) for j in jobs])
    for (x, y), (nets, st) in zip(sets, fleet):
        assert st['n_iter'] == [3, 3]
        for seed, net in zip([0, 1], nets):
            _close_to_oracle(net, mo.fit_network(x, y, seed, max_iter=3,
                                                 batch_size=1024), 3)
    monkeypatch.setenv('NB_TRAIN_NO_RESIDENT', '1')
    alone = emulator.train_ensembles([dict(j) for j in jobs])
    for (nets_a, _), (nets_b, _) in zip(fleet, alone):
        for a, b in zip(nets_a, nets_b):
            assert np.allclose(a.loss_curve_, b.loss_curve_, rtol=1e-12,
                               atol=0)
            for k in range(4):
                assert np.allclose(a.coefs_[k], b.coefs_[k], rtol=0,
                                   atol=1e-12)


def test_sampler_run_with_batch_size_1024():
    """``Sampler(..., neural_network_kwargs=dict(batch_size=1024))`` runs to
    the end, its emulators were trained with that batch, and the evidence of
    the README Gaussian comes out as with the default batch."""
    from nautilus_amd import GaussianLikelihood, Sampler, unit_prior
    like = GaussianLikelihood([0.4, 0.5, 0.6], 0.01 * np.eye(3))
    s = Sampler(unit_prior, like, n_dim=3, n_live=500, seed=1,
                neural_network_kwargs=dict(batch_size=1024))
    assert s.run(n_eff=2000, discard_exploration=True) is True
    nets = [net for b in s.bounds[1:] for nb in b.neural_bounds
            if nb.emulator is not None for net in nb.emulator.neural_networks]
    assert len(nets) >= 4
    assert all(net.sk_params == dict(batch_size=1024) for net in nets)
    assert abs(s.log_z - (-6.4e-5)) < 0.05
