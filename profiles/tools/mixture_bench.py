# Fused mixture likelihood (nb_mixture_loglike) on 65 536 points: time per
# call and the fractions of the fp64 MFMA peak (K D (D + 1) flop per point)
# and of the HBM peak (8 D + 8 bytes per point) DESIGN.md section 8 uses, at
# (D, K) = (50, 1), (50, 4), (50, 16), (100, 8); and, for the isotropic
# equal-weight mixture at (50, 4), the composition the legacy constructor
# runs (four GaussianLikelihood parts + torch.logsumexp) on the same inputs.
# Each figure is the median (min, max) of 20 calls timed one by one with
# device events after a warm-up.  Every shape runs in a child process of its
# own under a time limit; the first one that fails ends the run.
# usage: python profiles/tools/mixture_bench.py [--out FILE]
#        (default profiles/mixture/mixture_bench.txt)
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

N, REPEAT, WARMUP = 65536, 20, 5
PEAK_FLOPS, PEAK_BYTES = 78.6e12, 8e12
SHAPES = [(50, 1), (50, 4), (50, 16), (100, 8)]
STEP_SECONDS = 120


def timed(launch):
    import numpy as np
    import torch
    for _ in range(WARMUP):
        launch()
    torch.cuda.synchronize()
    ms = []
    for _ in range(REPEAT):
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        ev[0].record()
        launch()
        ev[1].record()
        ev[1].synchronize()
        ms.append(ev[0].elapsed_time(ev[1]))
    ms = np.array(ms) * 1e3
    return np.median(ms), ms.min(), ms.max()


def report(name, d, k, stat):
    med, lo, hi = stat
    flops = N * k * d * (d + 1) / (med * 1e-6)
    byts = N * (8 * d + 8) / (med * 1e-6)
    print('n=%d D=%d K=%d %-28s median %8.1f us (min %8.1f, max %8.1f)  '
          '%6.2f TFLOP/s = %.3f of MFMA peak, %7.1f GB/s = %.3f of HBM peak' % (
              N, d, k, name, med, lo, hi, flops / 1e12, flops / PEAK_FLOPS,
              byts / 1e9, byts / PEAK_BYTES), flush=True)
    return med


def problem(d, k, seed):
    import numpy as np
    rng = np.random.default_rng(seed)
    means = 0.25 + 0.5 * rng.random((k, d))
    covs = []
    for _ in range(k):
        q, _ = np.linalg.qr(rng.normal(size=(d, d)))
        ev = (0.01 + 0.03 * rng.random())**2 * np.logspace(0, -3, d)
        rng.shuffle(ev)
        covs.append((q * ev) @ q.T)
    w = rng.random(k) + 0.05
    return means, np.stack(covs), w / w.sum()


def step(d, k):
    import numpy as np
    import torch
    from nautilus_amd import GaussianMixtureLikelihood
    means, covs, w = problem(d, k, 100 * d + k)
    x = torch.rand((N, d), dtype=torch.float64, device='cuda')
    like = GaussianMixtureLikelihood(means, covs=covs, weights=w)
    report('fused', d, k, timed(lambda: like(x)))
    both = GaussianMixtureLikelihood(means, covs=covs, weights=w, labels=True)
    report('fused with labels', d, k, timed(lambda: both(x)))
    if (d, k) == (50, 4):
        sigma = 0.03
        legacy = GaussianMixtureLikelihood(means, sigma)
        fused = GaussianMixtureLikelihood(means, sigma, weights=np.ones(k))
        t_old = report('parts + logsumexp (legacy)', d, k,
                       timed(lambda: legacy(x)))
        t_new = report('fused, same mixture', d, k, timed(lambda: fused(x)))
        t_old2 = report('parts + logsumexp again', d, k,
                        timed(lambda: legacy(x)))
        diff = float((legacy(x) - fused(x)).abs().max())
        print('    legacy / fused = %.2f (%.2f on the second pass of the '
              'legacy path), max |legacy - fused| = %.3e' % (
                  t_old / t_new, t_old2 / t_new, diff), flush=True)


def main():
    out = os.path.join(ROOT, 'profiles', 'mixture', 'mixture_bench.txt')
    if '--out' in sys.argv:
        out = sys.argv[sys.argv.index('--out') + 1]
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, 'w') as f:
        for d, k in SHAPES:
            res = subprocess.run(
                [sys.executable, os.path.abspath(__file__), '--step', str(d),
                 str(k)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                timeout=STEP_SECONDS, text=True)
            sys.stdout.write(res.stdout)
            sys.stdout.flush()
            f.write(res.stdout)
            f.flush()
            if res.returncode != 0:
                sys.exit('step D=%d K=%d ended with status %d' % (
                    d, k, res.returncode))


if __name__ == '__main__':
    if '--step' in sys.argv:
        i = sys.argv.index('--step')
        step(int(sys.argv[i + 1]), int(sys.argv[i + 2]))
    else:
        main()
