# Fused Poisson likelihood behind a response matrix (nb_fold_poisson_loglike)
# against what the library offered before it, on the same n x K float64 source
# values: torch.matmul(s, R.T) into a preallocated n x P tensor (8 P bytes
# written per point), then nb_poisson_loglike on that tensor (8 P bytes read).
# n = 65 536; (K, P) = (16, 4096), (64, 4096), (1024, 1024), and (16, 2^20) for
# the fused kernel alone -- the baseline would need an n x P tensor of 512 GiB
# there.  Per shape the two are timed in turn, one call each per round, with
# device events around every call: 5 warm-up rounds, then 30 timed ones (10 at
# P = 2^20); each figure is the median (min, max).  TFLOP/s counts the 2 n P K
# flop of the product against the 78.6 TFLOP/s fp64 matrix peak of the MI355X.
# Every shape runs in a child process of its own under a time limit; the first
# one that fails ends the run.
# usage: python profiles/tools/fold_bench.py [--out FILE]
#        (default profiles/r08/fold_bench.txt)
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

WARMUP = 5
N = 1 << 16
SHAPES = [(16, 4096, 30, True), (64, 4096, 30, True), (1024, 1024, 30, True),
          (16, 1 << 20, 10, False)]
STEP_SECONDS = 240
PEAK_TFLOPS = 78.6


def timed(launches, repeat):
    """Median (min, max) in microseconds of each launch, taken in turn."""
    import numpy as np
    import torch
    for _ in range(WARMUP):
        for launch in launches:
            launch()
    torch.cuda.synchronize()
    ms = [[] for _ in launches]
    for _ in range(repeat):
        for i, launch in enumerate(launches):
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
            ev[0].record()
            launch()
            ev[1].record()
            ev[1].synchronize()
            ms[i].append(ev[0].elapsed_time(ev[1]))
    ms = np.array(ms) * 1e3
    return [(np.median(row), row.min(), row.max()) for row in ms]


def report(name, ks, p, stat, product=True):
    """``product`` says whether the timed call contains the 2 n P K flop."""
    med, lo, hi = stat
    line = 'K=%d P=%d n=%d %-40s median %10.1f us (min %10.1f, max %10.1f)' % (
        ks, p, N, name, med, lo, hi)
    if product:
        tflops = 2.0 * N * p * ks / (med * 1e-6) / 1e12
        line += ' %6.2f TFLOP/s = %4.1f %% of the fp64 matrix peak' % (
            tflops, 100 * tflops / PEAK_TFLOPS)
    print(line, flush=True)
    return med


def step(ks, p, repeat, baseline):
    import numpy as np
    import torch
    from nautilus_amd import device
    from nautilus_amd.likelihoods import poisson_log_const
    rng = np.random.default_rng(p + ks)
    resp = rng.random((p, ks)) * (rng.random((p, ks)) < 0.5)
    resp[np.arange(p), np.arange(p) % ks] += 0.25
    k = rng.poisson(50.0, size=p).astype(float)
    k[::7] = 0.0
    e = 50.0 / resp.sum(1)
    const = float(poisson_log_const(k).sum())
    gen = torch.Generator('cuda').manual_seed(p)
    s = torch.randn((N, ks), dtype=torch.float64, device='cuda', generator=gen)
    s.mul_(0.3).exp_()
    fused = device.FoldedPoissonTable(k, resp, exposure=e, log_const=const)
    launches = [lambda: fused.loglike(s)]
    if baseline:
        flat = device.PoissonTable(k, exposure=e, log_const=const)
        rt = torch.from_numpy(resp).cuda().t()
        mu = torch.empty((N, p), dtype=torch.float64, device='cuda')

        def composed():
            torch.matmul(s, rt, out=mu)
            return flat.loglike(mu)

        launches += [composed, lambda: torch.matmul(s, rt, out=mu),
                     lambda: flat.loglike(mu)]
    stats = timed(launches, repeat)
    t_new = report('fused nb_fold_poisson_loglike', ks, p, stats[0])
    if not baseline:
        print('    baseline not run: its n x P tensor would hold %.0f GiB'
              % (8.0 * N * p / 2**30), flush=True)
        return
    t_old = report('matmul(s, R.T) + nb_poisson_loglike', ks, p, stats[1])
    report('    matmul(s, R.T) alone', ks, p, stats[2])
    report('    nb_poisson_loglike alone', ks, p, stats[3], product=False)
    want, got = composed(), fused.loglike(s)
    rel = float(((got - want).abs() / want.abs()).max())
    print('    fused / baseline = %.3f, max relative difference %.2e' % (
        t_new / t_old, rel), flush=True)


def main():
    out = os.path.join(ROOT, 'profiles', 'r08', 'fold_bench.txt')
    if '--out' in sys.argv:
        out = sys.argv[sys.argv.index('--out') + 1]
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, 'w') as f:
        for ks, p, repeat, baseline in SHAPES:
            res = subprocess.run(
                [sys.executable, os.path.abspath(__file__), '--step', str(ks),
                 str(p), str(repeat), str(int(baseline))],
                stdout=subprocess.PIPE, timeout=STEP_SECONDS, text=True)
            sys.stdout.write(res.stdout)
            sys.stdout.flush()
            f.write(res.stdout)
            f.flush()
            if res.returncode != 0:
                sys.exit('step K=%d P=%d ended with status %d' % (
                    ks, p, res.returncode))


if __name__ == '__main__':
    if '--step' in sys.argv:
        i = sys.argv.index('--step')
        step(int(sys.argv[i + 1]), int(sys.argv[i + 2]), int(sys.argv[i + 3]),
             bool(int(sys.argv[i + 4])))
    else:
        main()
