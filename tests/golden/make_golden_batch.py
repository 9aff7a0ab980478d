"""Golden whole fits of the emulator at minibatches above the default 200 rows,
from the REFERENCE itself (``NeuralNetworkEmulator.train`` with
``neural_network_kwargs=dict(batch_size=...)``, i.e. scikit-learn's
MLPRegressor.fit), as ``make_golden.py`` writes them for the default batch.

Run in the build container only (the reference is not on the GPU box):

    OMP_NUM_THREADS=1 python tests/golden/make_golden_batch.py

Writes emulator_batch1000_D10_E2.npz (n = 5000, five full minibatches) and
emulator_batch4096_D6_E2.npz (n = 6100: one full minibatch and a ragged one).
Only data is stored."""

import os
import sys

import numpy as np

sys.path.insert(0, '/root/reference')
HERE = os.path.dirname(os.path.abspath(__file__))

import nautilus  # noqa: E402
from nautilus.neural import NeuralNetworkEmulator  # noqa: E402

assert nautilus.__version__ == '1.0.6'


def save(name, **arrays):
    path = os.path.join(HERE, name + '.npz')
    np.savez_compressed(path, **arrays)
    print('%-32s %8.1f KB' % (name, os.path.getsize(path) / 1024))


def emulator_batch_case(d, n, e, batch, seed):
    """The target of make_golden.emulator_case (rank of the radius)."""
    rng = np.random.default_rng(seed)
    x = rng.normal(size=(n, d))
    r = np.linalg.norm(x, axis=1)
    y = (np.argsort(np.argsort(-r)) + 0.5) / n
    emu = NeuralNetworkEmulator.train(
        x, y, n_networks=e, neural_network_kwargs=dict(batch_size=batch))
    test = rng.normal(size=(256, d))
    arrays = dict(x=x, y=y, mean=emu.mean, scale=emu.scale, test=test,
                  predict=emu.predict(test), n_networks=e, batch_size=batch)
    for i, net in enumerate(emu.neural_networks):
        assert net.batch_size == batch
        arrays['n_iter_%d' % i] = net.n_iter_
        arrays['loss_curve_%d' % i] = np.array(net.loss_curve_)
        for k in range(4):
            arrays['coef_%d_%d' % (i, k)] = net.coefs_[k]
            arrays['intercept_%d_%d' % (i, k)] = net.intercepts_[k]
    save('emulator_batch%d_D%d_E%d' % (batch, d, e), **arrays)


if __name__ == '__main__':
    emulator_batch_case(10, 5000, 2, 1000, 31)
    emulator_batch_case(6, 6100, 2, 4096, 32)
