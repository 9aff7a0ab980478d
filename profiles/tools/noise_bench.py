# Fused Gaussian likelihood with per-point noise parameters (nb_noise_loglike,
# both modes) against three baselines on the same n x P float64 tensors:
#   (a) the torch composition a user would write,
#       v = c sigma^2 + a + f m^2  (row mode; sigma^2 + w in full mode),
#       (-0.5 * ((m - d)**2 / v + torch.log(v))).sum(1);
#   (b) nb_poisson_loglike at the same shape (the streaming kernel this one
#       is modelled on: the same bytes, a log per element);
#   (c) a plain device copy of the tensor (dst.copy_(m): 8 P bytes read and
#       8 P written per point).
# P = 16, 256, 4096, 65536 with n P = 2^28 (a 2 GiB tensor; full mode reads
# two of them).  Per shape the launches are timed in turn, one call each per
# round, with device events around every call: 5 warm-up rounds, then 30
# timed ones; each figure is the median (min, max) of the 30.  GB/s counts the
# bytes the algorithm needs.  Every shape runs in a child process of its own
# under a time limit; the first one that fails ends the run.
# usage: python profiles/tools/noise_bench.py [--out FILE]
#        (default profiles/r07/noise_bench.txt)
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
    print('P=%d n=%d %-46s median %9.1f us (min %9.1f, max %9.1f) '
          '%7.1f GB/s' % (p, n, name, med, lo, hi,
                          byts / (med * 1e-6) / 1e9), flush=True)
    return med


def step(p, n):
    import numpy as np
    import torch
    from nautilus_amd import device
    rng = np.random.default_rng(p)
    d = rng.normal(size=p)
    s2 = (0.5 + rng.random(p))**2
    d_dev, s2_dev = torch.from_numpy(d).cuda(), torch.from_numpy(s2).cuda()
    gen = torch.Generator('cuda').manual_seed(p)
    m = torch.randn((n, p), dtype=torch.float64, device='cuda', generator=gen)
    m.add_(d_dev)
    coef = torch.rand((n, 3), dtype=torch.float64, device='cuda',
                      generator=gen)
    coef[:, 0] += 0.5
    coef[:, 2] *= 0.1
    table = device.NoiseTable(d, s2, log_norm=-0.5 * p * np.log(2 * np.pi))
    k = rng.poisson(50.0, size=p).astype(float)
    poisson = device.PoissonTable(k)
    rates = m.abs().add_(1.0)               # what the Poisson kernel reads
    dst = torch.empty_like(m)
    table_norm = -0.5 * p * np.log(2 * np.pi)

    def composition_row():
        v = coef[:, 0:1] * s2_dev + coef[:, 1:2] + coef[:, 2:3] * m * m
        return table_norm + (-0.5 * ((m - d_dev)**2 / v + torch.log(v))).sum(1)

    stats = timed([lambda: table.loglike(m, coef, device.NOISE_ROW),
                   composition_row, lambda: poisson.loglike(rates),
                   lambda: dst.copy_(m)])
    t_row = report('fused nb_noise_loglike, row mode', p, n, stats[0],
                   n * (8 * p + 32))
    t_old = report('torch composition, row mode', p, n, stats[1],
                   n * (8 * p + 32))
    t_poi = report('fused nb_poisson_loglike', p, n, stats[2],
                   n * (8 * p + 8))
    t_copy = report('torch dst.copy_(m)', p, n, stats[3], n * 16 * p)
    want = composition_row()
    got = table.loglike(m, coef, device.NOISE_ROW)
    rel = float(((got - want).abs() / want.abs()).max())
    print('    row mode: torch / fused = %.2f, fused / poisson = %.2f, fused '
          '/ copy = %.2f, max relative difference %.2e' % (
              t_old / t_row, t_row / t_poi, t_row / t_copy, rel), flush=True)
    del want, got, rates
    # full mode: dst becomes the (n, P) noise, positive
    dst.copy_(m).sub_(d_dev).pow_(2).mul_(0.1).add_(0.01)

    def composition_full():
        v = s2_dev + dst
        return table_norm + (-0.5 * ((m - d_dev)**2 / v + torch.log(v))).sum(1)

    stats = timed([lambda: table.loglike(m, dst, device.NOISE_FULL),
                   composition_full])
    t_full = report('fused nb_noise_loglike, full mode', p, n, stats[0],
                    n * (16 * p + 8))
    t_old = report('torch composition, full mode', p, n, stats[1],
                   n * (16 * p + 8))
    want = composition_full()
    got = table.loglike(m, dst, device.NOISE_FULL)
    rel = float(((got - want).abs() / want.abs()).max())
    print('    full mode: torch / fused = %.2f, fused / copy = %.2f, max '
          'relative difference %.2e' % (t_old / t_full, t_full / t_copy, rel),
          flush=True)


def main():
    out = os.path.join(ROOT, 'profiles', 'r07', 'noise_bench.txt')
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
