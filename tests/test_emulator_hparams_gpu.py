"""The device trainer (nb_mlp_train.hip) away from the default
hyper-parameters: Adam's ``beta_1`` / ``beta_2`` / ``epsilon`` / learning
rate in the update and in the step size (carried as beta^t from step to step
by the resident kernel, ``pow`` per step by the two-launch kernels), and the
stopping rule (``tol``, ``n_iter_no_change``, ``max_iter``) -- with stops
inside, at the end of and behind the first 16-epoch launch.  GPU only.

Judges: scikit-learn's ``MLPRegressor.fit`` for whole fits through
``NeuralNetworkEmulator.train``; the oracle's ``fit_network`` -- which equals
scikit-learn bit for bit at these options, test_emulator_hparams_cpu.py --
where ``train_networks`` / ``train_ensembles`` are driven directly.

Every case recomputes the stop margin of ITS reference (hparam_cases.
stop_margin) and asserts it is at least MIN_MARGIN, a million times the
tolerance of the loss curve: equal stop epochs are then a fair demand.

Every comparison prints its largest deviations before it asserts (-s shows
them)."""

import numpy as np
import pytest
import torch

import hparam_cases as hc

pytestmark = pytest.mark.gpu

# device against oracle, as in test_hip_parity.py::
# test_emulator_training_matches_oracle
LOSS_RTOL = 1e-9
WEIGHT_ATOL = 1e-8
PREDICT_ATOL = 1e-7
MIN_MARGIN = 1e-3


@pytest.fixture(scope='module')
def dev():
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    from nautilus_amd import device
    return device


def _cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _rank_target(r):
    """Descending rank over n, the sampler's kind of target."""
    return np.argsort(np.argsort(-r)) / len(r)


def _check(label, net, n_iter, curve, coefs, intercepts, kw):
    """One device network against its reference fit."""
    margin = hc.stop_margin(curve, kw)
    got = np.asarray(net.loss_curve_)
    m = min(len(got), len(curve))
    d_loss = (np.max(np.abs(got[:m] / np.asarray(curve)[:m] - 1))
              if m else np.inf)
    d_w = max(np.max(np.abs(a - b)) for a, b in
              zip(list(net.coefs_) + list(net.intercepts_),
                  list(coefs) + list(intercepts)))
    print('%-28s n_iter %3d (ref %3d)  margin %.1e  loss %.2e  weights %.2e'
          % (label, net.n_iter_, n_iter, margin, d_loss, d_w))
    assert margin >= MIN_MARGIN
    assert net.n_iter_ == n_iter == len(curve)
    assert np.allclose(got, curve, rtol=LOSS_RTOL, atol=0)
    for k in range(4):
        assert np.allclose(net.coefs_[k], coefs[k], rtol=0, atol=WEIGHT_ATOL)
        assert np.allclose(net.intercepts_[k], intercepts[k], rtol=0,
                           atol=WEIGHT_ATOL)


def _check_sklearn(label, net, sk, kw):
    _check(label, net, sk.n_iter_, sk.loss_curve_, sk.coefs_, sk.intercepts_,
           kw)


def _check_oracle(label, net, ref, kw):
    _check(label, net, ref.n_iter, ref.loss_curve, ref.coefs, ref.intercepts,
           kw)


def _train_d5(name, seeds=4, **extra):
    from nautilus_amd.emulator import NeuralNetworkEmulator
    g = hc.load_golden('emulator_D5_E1')
    return NeuralNetworkEmulator.train(
        g['x'], g['y'], n_networks=seeds,
        neural_network_kwargs=dict(hc.SETS[name], **extra))


@pytest.mark.parametrize('name', sorted(hc.SETS))
def test_whole_fit_equals_sklearn(dev, name):
    """Seeds 0-3 in one trainer: stop epochs network by network (for A:
    16 / 17 / 14 / 18 -- network 2 stops inside the first launch and sits
    stopped through the second, network 0 stops at its last epoch), loss
    curves, weights, and the prediction of the ensemble."""
    g = hc.load_golden('emulator_D5_E1')
    kw = hc.SETS[name]
    emu = _train_d5(name)
    assert np.allclose(emu.mean, g['mean'], rtol=1e-14, atol=1e-15)
    assert np.allclose(emu.scale, g['scale'], rtol=1e-13)
    fits = [hc.d5_sklearn(name, seed) for seed in range(4)]
    assert [f.n_iter_ for f in fits] == hc.STOPS[name]
    for seed, (net, sk) in enumerate(zip(emu.neural_networks, fits)):
        _check_sklearn('%s seed %d' % (name, seed), net, sk, kw)
    assert emu.trainer_stats['n_iter'] == hc.STOPS[name]
    probe = np.random.default_rng(1).random((2000, 5))
    xs = (probe - g['mean']) / g['scale']
    want = np.mean([sk.predict(xs) for sk in fits], axis=0)
    got = emu.predict(probe)
    print('%s predict %.2e' % (name, np.max(np.abs(got - want))))
    assert np.allclose(got, want, rtol=0, atol=PREDICT_ATOL)


@pytest.mark.parametrize('name', ['A', 'C'])
def test_both_step_size_paths(dev, name, monkeypatch, capfd):
    """The resident kernel (beta^t carried from step to step) and the
    two-launch kernels (NB_TRAIN_TWO_LAUNCH: ``pow`` every step) against
    scikit-learn, and against each other in their stop epochs.  The
    trainer's own report (NB_TRAIN_DEBUG) tells that each run took the path
    it is meant to test."""
    kw = hc.SETS[name]
    fits = [hc.d5_sklearn(name, seed) for seed in range(4)]
    monkeypatch.setenv('NB_TRAIN_DEBUG', '1')
    capfd.readouterr()
    resident = _train_d5(name)
    assert 'two_launch=0' in capfd.readouterr().err
    monkeypatch.setenv('NB_TRAIN_TWO_LAUNCH', '1')
    two = _train_d5(name)
    assert 'two_launch=1' in capfd.readouterr().err
    for seed, sk in enumerate(fits):
        _check_sklearn('%s seed %d resident' % (name, seed),
                       resident.neural_networks[seed], sk, kw)
        _check_sklearn('%s seed %d two-launch' % (name, seed),
                       two.neural_networks[seed], sk, kw)
    assert two.trainer_stats['n_iter'] == resident.trainer_stats['n_iter'] \
        == hc.STOPS[name]


def test_large_minibatch_layout(dev):
    """Set B at batch 512 (the LARGE instantiations of the kernels): two
    steps per epoch, of 512 and 488 rows."""
    kw = dict(hc.SETS['B'], batch_size=512)
    emu = _train_d5('B', seeds=3, batch_size=512)
    fits = [hc.d5_sklearn('B', seed, 512) for seed in range(3)]
    assert [f.n_iter_ for f in fits] == [12, 7, 7]
    for seed, (net, sk) in enumerate(zip(emu.neural_networks, fits)):
        assert net.sk_params['batch_size'] == 512
        assert sk.t_ == sk.n_iter_ * 1000 == net.t_
        _check_sklearn('B batch 512 seed %d' % seed, net, sk, kw)


@pytest.fixture(scope='module')
def drawn_sets():
    """The training sets that are not the fixture's, drawn from ONE generator
    in this order: the fleet's 700 x 6 and 450 x 6 (inputs, then the noise of
    the target), then the 437 x 65 of the wide first layer."""
    rng = np.random.default_rng(4)
    fleet = []
    for n in (700, 450):
        x = rng.normal(size=(n, 6))
        r = np.linalg.norm(x[:, :3], axis=1) + 0.3 * rng.normal(size=n)
        fleet.append((x, _rank_target(r)))
    x = rng.normal(size=(437, 65))
    wide = (x, _rank_target(np.linalg.norm(x[:, :8], axis=1)))
    return fleet, wide


@pytest.fixture(scope='module')
def fleet_sets(drawn_sets):
    """Two training sets of 700 x 6 and 450 x 6 rows and the oracle's fits
    of seeds 0 and 1 on each, for sets A and B."""
    from oracle import mlp_oracle as mo
    sets = drawn_sets[0]
    refs = {(name, j, seed): mo.fit_network(x, y, seed,
                                            **hc.oracle_kwargs(hc.SETS[name]))
            for name in 'AB' for j, (x, y) in enumerate(sets)
            for seed in (0, 1)}
    assert [refs['A', j, s].n_iter for j in (0, 1) for s in (0, 1)] == \
        [23, 32, 47, 33]
    assert [refs['B', j, s].n_iter for j in (0, 1) for s in (0, 1)] == \
        [9, 9, 7, 9]
    return sets, refs


def _fleet_jobs(sets, names):
    return [dict(xs=_cuda(x), y=_cuda(y), seeds=[0, 1],
                 hparams=hc.device_hparams(hc.SETS[name]))
            for (x, y), name in zip(sets, names)]


def _check_fleet(label, out, refs, names):
    for j, ((nets, stats), name) in enumerate(zip(out, names)):
        for seed, net in zip((0, 1), nets):
            _check_oracle('%s job %d %s seed %d' % (label, j, name, seed),
                          net, refs[name, j, seed], hc.SETS[name])
        assert stats['n_iter'] == [refs[name, j, s].n_iter for s in (0, 1)]


@pytest.mark.parametrize('names', ['AA', 'BB', 'AB'])
def test_fleet_with_different_training_sets(dev, fleet_sets, names):
    """Two ensembles with a training set each.  Equal hyper-parameters: one
    fleet trainer, the four networks in one resident launch with their own
    row counts (4 and 3 steps per epoch) and stop epochs from 23 to 47.
    A for one and B for the other: a trainer and a stream per ensemble."""
    from nautilus_amd import emulator
    sets, refs = fleet_sets
    out = emulator.train_ensembles(_fleet_jobs(sets, names))
    _check_fleet('fleet ' + names, out, refs, names)


def test_fleet_without_the_resident_kernel(dev, fleet_sets, monkeypatch):
    """The A / A fleet where the library cannot provide the resident kernel
    (NB_TRAIN_NO_RESIDENT): a trainer per ensemble, two launches per step."""
    from nautilus_amd import emulator
    sets, refs = fleet_sets
    monkeypatch.setenv('NB_TRAIN_NO_RESIDENT', '1')
    out = emulator.train_ensembles(_fleet_jobs(sets, 'AA'))
    _check_fleet('no resident AA', out, refs, 'AA')


def test_wide_first_layer(dev, drawn_sets):
    """Set A at 65 inputs (five k-tiles in layer 1: another job list of the
    gradient phase, whose jobs all apply Adam's constants) and 437 rows
    (three steps per epoch, the last of 37 rows)."""
    from nautilus_amd import emulator
    from oracle import mlp_oracle as mo
    kw = hc.SETS['A']
    x, y = drawn_sets[1]
    nets, stats = emulator.train_networks(_cuda(x), _cuda(y), [0, 3],
                                          hparams=hc.device_hparams(kw))
    refs = [mo.fit_network(x, y, seed, **hc.oracle_kwargs(kw))
            for seed in (0, 3)]
    assert [r.n_iter for r in refs] == [37, 32]
    for seed, net, ref in zip((0, 3), nets, refs):
        _check_oracle('wide seed %d' % seed, net, ref, kw)


def test_set_hparams_refusal_leaves_the_trainer_as_it_was(dev):
    """``nb_trainer_set_hparams`` with batch = 0 and with max_iter = 10001
    returns NB_ERR_UNSUPPORTED and stores NOTHING of the call -- whose other
    arguments are far from the defaults here --: three epochs afterwards are
    those of the default fit."""
    from nautilus_amd import _lib, emulator
    from oracle import mlp_oracle as mo
    x, y = hc.d5_data()
    n = len(x)
    seeds = [0, 1]
    init, perms = [], []
    for seed in seeds:
        rs = np.random.RandomState(seed)
        init.append(emulator._glorot(5, rs))
        order, eps = np.arange(n), []
        for _ in range(3):
            order = mo.epoch_permutation(rs, order)
            eps.append(order)
        perms.append(eps)
    trainer = emulator.Trainer(_cuda(x), _cuda(y), init)
    try:
        lib = _lib.load()
        for batch, max_iter in [(0, 10000), (50, 10001)]:
            status = lib.nb_trainer_set_hparams(
                trainer._h, 0.5, 0.1, 0.2, 1.0, batch, max_iter, 1, 5.0)
            assert status == _lib.ERR_UNSUPPORTED
            assert b'max_iter' in lib.nb_last_error()
        status = trainer.run(np.array(perms, dtype=np.int32))
        assert list(status) == [3, 3]
        for i, seed in enumerate(seeds):
            ref = mo.fit_network(x, y, seed, max_iter=3)
            coefs, intercepts = trainer.weights(i)
            net = emulator.Network(coefs, intercepts, int(status[i]),
                                   trainer.loss_curve(i, 3))
            # (three epochs of the default fit: the rule cannot fire)
            _check_oracle('after refusal seed %d' % seed, net, ref,
                          dict(max_iter=3))
    finally:
        trainer.close()
