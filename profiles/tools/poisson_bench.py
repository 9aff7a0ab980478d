# Fused Poisson likelihood of binned counts (nb_poisson_loglike) against two
# baselines that do not involve it, on the same n x P float64 tensor:
#   * the torch composition a user would write,
#     (torch.xlogy(k, mu) - mu - torch.lgamma(k + 1)).sum(1);
#   * a plain device copy of the tensor (dst.copy_(m): 8 P bytes read and 8 P
#     written per point), the HBM floor.
# P = 16, 256, 4096, 65536 with n P = 2^28 (a 2 GiB tensor).  Per shape the
# three are timed in turn, one call each per round, with device events around
# every call: 5 warm-up rounds, then 30 timed ones; each figure is the median
# (min, max) of the 30.  GB/s counts the bytes the algorithm needs (8 P + 8
# per point for the likelihoods, 16 P for the copy).  Every shape runs in a
# child process of its own under a time limit; the first one that fails ends
# the run.
# usage: python profiles/tools/poisson_bench.py [--out FILE]
#        (default profiles/r07/poisson_bench.txt)
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

REPEAT, WARMUP = 30, 5
SHAPES = [(16, 1 << 24), (256, 1 << 20), (4096, 1 << 16), (65536, 1 << 12)]
STEP_SECONDS = 240


def timed(launches):
    """Median (min, max) in microseconds of each launch, taken in turn."""
    import numpy as np
    import torch
    for _ in range(WARMUP):
        for launch in launches:
            launch()
    torch.cuda.synchronize()
    ms = [[] for _ in launches]
    for _ in range(REPEAT):
        for i, launch in enumerate(launches):
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
            ev[0].record()
            launch()
            ev[1].record()
            ev[1].synchronize()
            ms[i].append(ev[0].elapsed_time(ev[1]))
    ms = np.array(ms) * 1e3
    return [(np.median(row), row.min(), row.max()) for row in ms]


def report(name, p, n, stat, byts):
    med, lo, hi = stat
    print('P=%d n=%d %-44s median %9.1f us (min %9.1f, max %9.1f) '
          '%7.1f GB/s' % (p, n, name, med, lo, hi,
                          byts / (med * 1e-6) / 1e9), flush=True)
    return med


def step(p, n):
    import numpy as np
    import torch
    from nautilus_amd import device
    from nautilus_amd.likelihoods import poisson_log_const
    rng = np.random.default_rng(p)
    k = rng.poisson(50.0, size=p).astype(float)
    k[::7] = 0.0
    k_dev = torch.from_numpy(k).cuda()
    gen = torch.Generator('cuda').manual_seed(p)
    m = torch.randn((n, p), dtype=torch.float64, device='cuda', generator=gen)
    m.mul_(0.3).exp_().mul_(k_dev + 1.0)
    dst = torch.empty_like(m)
    table = device.PoissonTable(
        k, log_const=float(poisson_log_const(k).sum()))

    def composition():
        return (torch.xlogy(k_dev, m) - m - torch.lgamma(k_dev + 1)).sum(1)

    stats = timed([lambda: table.loglike(m), composition,
                   lambda: dst.copy_(m)])
    t_new = report('fused nb_poisson_loglike', p, n, stats[0], n * (8 * p + 8))
    t_old = report('torch (xlogy(k, mu) - mu - lgamma(k + 1)).sum(1)', p, n,
                   stats[1], n * (8 * p + 8))
    t_copy = report('torch dst.copy_(m)', p, n, stats[2], n * 16 * p)
    want = composition()
    got = table.loglike(m)
    rel = float(((got - want).abs() / want.abs()).max())
    print('    torch / fused = %.2f, fused / copy = %.2f, max relative '
          'difference %.2e' % (t_old / t_new, t_new / t_copy, rel), flush=True)


def main():
    out = os.path.join(ROOT, 'profiles', 'r07', 'poisson_bench.txt')
    if '--out' in sys.argv:
        out = sys.argv[sys.argv.index('--out') + 1]
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, 'w') as f:
        for p, n in SHAPES:
            res = subprocess.run(
                [sys.executable, os.path.abspath(__file__), '--step', str(p),
                 str(n)], stdout=subprocess.PIPE, timeout=STEP_SECONDS,
                text=True)
            sys.stdout.write(res.stdout)
            sys.stdout.flush()
            f.write(res.stdout)
            f.flush()
            if res.returncode != 0:
                sys.exit('step P=%d n=%d ended with status %d' % (
                    p, n, res.returncode))


if __name__ == '__main__':
    if '--step' in sys.argv:
        i = sys.argv.index('--step')
        step(int(sys.argv[i + 1]), int(sys.argv[i + 2]))
    else:
        main()
