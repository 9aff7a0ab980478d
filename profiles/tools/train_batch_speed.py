"""Step and epoch time of the emulator trainer against the minibatch size.

For (n_dim, networks) = (50, 4) and (100, 8) on 100 000 rows, batches 200,
1000, 2000 and 4096: one trainer per case, one warm-up epoch, then EPOCHS
epochs timed with device-synchronised wall clocks around nb_trainer_run
(fixed row orders, no early stop).  Prints one JSON line per case:
ms per epoch, us per Adam step, steps per epoch, path (resident or two
launches).  Usage:

    python profiles/tools/train_batch_speed.py [--epochs 3] [--out FILE]
"""

import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(
    os.path.abspath(__file__)))))

from nautilus_amd import emulator  # noqa: E402


def case(d, e, n, batch, epochs):
    rng = np.random.default_rng(d)
    x = torch.from_numpy(rng.normal(size=(n, d))).cuda()
    y = torch.from_numpy(rng.random(n)).cuda()
    nets = [emulator._glorot(d, np.random.RandomState(i)) for i in range(e)]
    tr = emulator.Trainer(x, y, nets, dict(batch=batch, max_iter=10000,
                                           n_iter_no_change=10000))
    perms = np.stack([np.stack([rng.permutation(n).astype(np.int32)
                                for _ in range(epochs)]) for _ in range(e)])
    tr.run(perms[:, :1])                              # warm-up epoch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    status = tr.run(perms)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    assert np.all(status == 1 + epochs), status
    steps = -(-n // batch)
    tr.close()
    return dict(n_dim=d, networks=e, rows=n, batch=batch, epochs=epochs,
                ms_per_epoch=1e3 * dt / epochs,
                us_per_step=1e6 * dt / (epochs * steps), steps_per_epoch=steps)


def main():
    p = argparse.ArgumentParser()
    p.add_argument('--epochs', type=int, default=3)
    p.add_argument('--rows', type=int, default=100000)
    p.add_argument('--out', default=None)
    a = p.parse_args()
    lines = []
    for d, e in [(50, 4), (100, 8)]:
        for batch in (200, 1000, 2000, 4096):
            r = case(d, e, a.rows, batch, a.epochs)
            print(json.dumps(r), flush=True)
            lines.append(r)
    if a.out:
        with open(a.out, 'w') as f:
            for r in lines:
                f.write(json.dumps(r) + '\n')


if __name__ == '__main__':
    main()
