# Fused Gaussian likelihood with outliers (nb_outlier_loglike) against three
# baselines on the same n x P float64 tensor:
#   (a) the stable torch composition a careful user would write,
#       v = c sigma^2 + a + f m^2,  u = sigma^2 + s,
#       l1 = log1p(-p) - 0.5 log v - 0.5 (m - d)^2 / v,
#       l2 = log p     - 0.5 log u - 0.5 (d - b)^2 / u,
#       torch.logaddexp(l1, l2).sum(1);
#   (b) nb_noise_loglike in row mode at the same shape, on the first three
#       columns of the same coefficients read in place (the same bytes, less
#       arithmetic: what the mixture costs);
#   (c) a plain device copy of the tensor (dst.copy_(m): 8 P bytes read and
#       8 P written per point).
# P = 16, 256, 4096, 65536 with n P = 2^28 (a 2 GiB tensor).  Per shape the
# launches are timed in turn, one call each per round, with device events
# around every call: 5 warm-up rounds, then 30 timed ones; each figure is the
# median (min, max) of the 30.  GB/s counts the bytes the algorithm needs.
# Every shape runs in a child process of its own under a time limit; the first
# one that fails ends the run.
# usage: python profiles/tools/outlier_bench.py [--out FILE]
#        (default profiles/r08/outlier_bench.txt)
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
    # one measurement in sixteen lies 5 to 25 error bars away
    m.add_((torch.rand((n, p), dtype=torch.float64, device='cuda',
                       generator=gen) < 1 / 16) *
           (5.0 + 20.0 * torch.rand((n, p), dtype=torch.float64,
                                    device='cuda', generator=gen)))
    coef = torch.rand((n, 6), dtype=torch.float64, device='cuda',
                      generator=gen)
    coef[:, 0] += 0.5                       # c
    coef[:, 2] *= 0.01                      # f
    coef[:, 3] *= 0.5                       # p in [0, 1/2)
    coef[:, 4] -= 0.5                       # b
    coef[:, 5] = 10.0 + 90.0 * coef[:, 5]   # s
    table_norm = -0.5 * p * np.log(2 * np.pi)
    table = device.NoiseTable(d, s2, log_norm=table_norm)
    dst = torch.empty_like(m)
    cut = coef[:, :3]                       # (c, a, f) in place, ld_noise 6

    def composition():
        v = coef[:, 0:1] * s2_dev + coef[:, 1:2] + coef[:, 2:3] * m * m
        u = s2_dev + coef[:, 5:6]
        l1 = torch.log1p(-coef[:, 3:4]) - 0.5 * torch.log(v) - \
            0.5 * (m - d_dev)**2 / v
        l2 = torch.log(coef[:, 3:4]) - 0.5 * torch.log(u) - \
            0.5 * (d_dev - coef[:, 4:5])**2 / u
        return table_norm + torch.logaddexp(l1, l2).sum(1)

    stats = timed([lambda: table.outlier_loglike(m, coef), composition,
                   lambda: table.loglike(m, cut, device.NOISE_ROW),
                   lambda: dst.copy_(m)])
    t_new = report('fused nb_outlier_loglike', p, n, stats[0],
                   n * (8 * p + 56))
    t_old = report('torch composition (logaddexp)', p, n, stats[1],
                   n * (8 * p + 56))
    t_noise = report('fused nb_noise_loglike, row mode', p, n, stats[2],
                     n * (8 * p + 32))
    t_copy = report('torch dst.copy_(m)', p, n, stats[3], n * 16 * p)
    want = composition()
    got = table.outlier_loglike(m, coef)
    rel = float(((got - want).abs() / want.abs()).max())
    print('    torch / fused = %.2f, fused / noise = %.2f, fused / copy = '
          '%.2f, %.1f ps per element, max relative difference %.2e' % (
              t_old / t_new, t_new / t_noise, t_new / t_copy,
              t_new * 1e6 / (n * p), rel), flush=True)


def main():
    out = os.path.join(ROOT, 'profiles', 'r08', 'outlier_bench.txt')
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
