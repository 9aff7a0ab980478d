"""``batch_size`` of ``neural_network_kwargs``: scikit-learn's rules (an
integer >= 1 or 'auto' = min(200, n); a value above n is clipped with
scikit-learn's warning) plus the device trainer's cap, checked at
``Sampler.__init__`` and at ``NeuralNetworkEmulator.train``.  CPU only."""

import warnings

import numpy as np
import pytest

from nautilus_amd import emulator


def test_batch_size_translation():
    hp = emulator._hparams_from_kwargs
    assert hp(dict(batch_size='auto')) == dict(batch=200)
    assert hp(dict(batch_size=1)) == dict(batch=1)
    assert hp(dict(batch_size=1000)) == dict(batch=1000)
    assert hp(dict(batch_size=np.int64(2000))) == dict(batch=2000)
    assert hp(dict(batch_size=emulator.MAX_BATCH)) == \
        dict(batch=emulator.MAX_BATCH)
    # no default batch key
    assert hp(dict(max_iter=5)) == dict(max_iter=5)


@pytest.mark.parametrize('bad', [0, -1, True, False, 1.5, 200.0, 'big', None,
                                 emulator.MAX_BATCH + 1])
def test_bad_batch_size_is_refused_early(bad):
    with pytest.raises(ValueError, match='batch_size'):
        emulator._hparams_from_kwargs(dict(batch_size=bad))
    with pytest.raises(ValueError, match='batch_size'):
        emulator.check_network_kwargs(dict(batch_size=bad))
    # NeuralNetworkEmulator.train refuses it before touching the data
    with pytest.raises(ValueError, match='batch_size'):
        emulator.NeuralNetworkEmulator.train(
            np.zeros((10, 2)), np.zeros(10),
            neural_network_kwargs=dict(batch_size=bad))


def test_cap_is_named():
    with pytest.raises(ValueError, match=str(emulator.MAX_BATCH)):
        emulator.check_network_kwargs(dict(batch_size=10 ** 6))


def test_sampler_refuses_a_bad_batch_size_at_init():
    from nautilus_amd import GaussianLikelihood, Sampler, unit_prior
    like = GaussianLikelihood([0.5, 0.5], 0.01 * np.eye(2))
    with pytest.raises(ValueError, match='batch_size'):
        Sampler(unit_prior, like, n_dim=2, n_live=100,
                neural_network_kwargs=dict(batch_size=0))


def test_batch_size_above_n_is_clipped_with_sklearns_warning():
    with pytest.warns(UserWarning, match='It is going to be clipped'):
        emulator._warn_batch_clip(dict(batch_size=500), 300)
    with warnings.catch_warnings():
        warnings.simplefilter('error')
        emulator._warn_batch_clip(dict(batch_size=300), 300)
        emulator._warn_batch_clip(dict(batch_size='auto'), 10)
        emulator._warn_batch_clip(dict(), 10)


def test_header_cap_matches():
    import os
    import re
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(root, 'include', 'nautilus_hip.h')) as f:
        m = re.search(r'#define NB_TRAIN_MAX_BATCH (\d+)', f.read())
    assert m and int(m.group(1)) == emulator.MAX_BATCH
