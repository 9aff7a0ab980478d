"""Time of one ``GaussianLikelihood`` call (r2 of a bound without emulators,
then two elementwise torch kernels) with HIP events: REPEATS repeats of CALLS
back-to-back calls per row count, at n_dim 50.  Run from the repository root:

    python profiles/tools/geom_time.py [rows ...]      (default 65536 1048576)

NAUTILUS_HIP_LIB selects the build of the library that is measured."""

import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(
    os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from nautilus_amd.likelihoods import GaussianLikelihood      # noqa: E402

REPEATS, CALLS, D = 5, 200, 50


def main():
    rows = [int(a) for a in sys.argv[1:]] or [65536, 1 << 20]
    rng = np.random.default_rng(1)
    a = rng.normal(size=(D, D))
    like = GaussianLikelihood(np.full(D, 0.5), 0.01 * (a @ a.T / D + np.eye(D)))
    print('library:', os.environ.get('NAUTILUS_HIP_LIB', 'default'))
    for n in rows:
        x = torch.rand((n, D), dtype=torch.float64, device='cuda')
        for _ in range(20):
            like(x)
        times = []
        for _ in range(REPEATS):
            t0 = torch.cuda.Event(enable_timing=True)
            t1 = torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            t0.record()
            for _ in range(CALLS):
                like(x)
            t1.record()
            t1.synchronize()
            times.append(t0.elapsed_time(t1) / CALLS)
        print('n %8d: ms per call, %d repeats of %d calls: %s  median %.4f  '
              'slowest %.4f' % (n, REPEATS, CALLS,
                                ' '.join('%.4f' % t for t in times),
                                float(np.median(times)), max(times)))


if __name__ == '__main__':
    main()
