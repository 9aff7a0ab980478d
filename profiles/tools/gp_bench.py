# Fused Gaussian-process likelihood (nb_gp_loglike, both modes) against what a
# user writes without it on the same inputs on the same GPU: a device callable
# that builds the (n, P, P) covariances with torch (a rho(D / l) + diag(sigma^2
# + s); in full mode C + diag(sigma^2) alone) and calls
# torch.linalg.cholesky_ex, torch.linalg.solve_triangular and a log of the
# diagonal.
# P = 16, 32, 64, 128 with n = 8192, the Matern-3/2 function.  Per shape the
# launches are timed in turn, one call each per round, with device events
# around every call: 5 warm-up rounds, then 30 timed ones; each figure is the
# median (min, max) of the 30.  GFLOP/s counts the P^3 / 3 flops of the
# factorisation per point and is also given as a fraction of the fp64 MFMA
# peak the library measures on the same device (nb_mfma_f64_peak).  Every shape
# runs in a child process of its own under a time limit; the first one that
# fails ends the run.
# usage: python profiles/tools/gp_bench.py [--out FILE]
#        (default profiles/r07/gp_bench.txt)
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

REPEAT, WARMUP = 30, 5
SHAPES = [(16, 8192), (32, 8192), (64, 8192), (128, 8192)]
STEP_SECONDS = 240
SQRT3 = 3.0**0.5


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


def report(name, p, n, stat, peak):
    med, lo, hi = stat
    gflops = n * p**3 / 3.0 / (med * 1e-6) / 1e9
    print('P=%d n=%d %-44s median %9.1f us (min %9.1f, max %9.1f) %8.1f '
          'GFLOP/s = %.4f of the fp64 MFMA peak, %6.3f us per point' % (
              p, n, name, med, lo, hi, gflops, gflops / (peak * 1e3),
              med / n), flush=True)
    return med


def step(p, n):
    import numpy as np
    import torch
    from nautilus_amd import device
    peak = device.mfma_f64_peak()
    rng = np.random.default_rng(p)
    t = np.sort(rng.uniform(0, 10, size=p))
    dist = np.abs(t[:, None] - t[None, :])
    d = rng.normal(size=p)
    s2 = (0.05 + 0.1 * rng.random(p))**2
    log_norm = -0.5 * p * np.log(2 * np.pi)
    table = device.GPTable(d, s2, dist, kernel='matern32', log_norm=log_norm)
    d_dev, s2_dev, dist_dev = (torch.from_numpy(a).cuda()
                               for a in (d, s2, dist))
    gen = torch.Generator('cuda').manual_seed(p)
    m = torch.randn((n, p), dtype=torch.float64, device='cuda', generator=gen)
    m.add_(d_dev)
    h = torch.rand((n, 3), dtype=torch.float64, device='cuda', generator=gen)
    h[:, 0] += 0.5                               # a in [0.5, 1.5)
    h[:, 1] = 0.3 + 2.0 * h[:, 1]                # l in [0.3, 2.3)
    h[:, 2] = 0.01 + 0.1 * h[:, 2]               # s in [0.01, 0.11)
    eye = torch.eye(p, dtype=torch.float64, device='cuda')

    def covariance():
        u = SQRT3 * dist_dev / h[:, 1, None, None]
        return h[:, 0, None, None] * (1 + u) * torch.exp(-u) + \
            h[:, 2, None, None] * eye

    def finish(k):
        chol, _ = torch.linalg.cholesky_ex(k + torch.diag(s2_dev))
        y = torch.linalg.solve_triangular(chol, (m - d_dev).unsqueeze(2),
                                          upper=False)
        log_det = 2 * torch.log(torch.diagonal(chol, dim1=1, dim2=2)).sum(1)
        return log_norm - 0.5 * ((y * y).sum((1, 2)) + log_det)

    c = covariance()
    print('fp64 MFMA peak %.1f TFLOP/s' % peak, flush=True)
    stats = timed([lambda: table.loglike(m, h, device.GP_HYPER),
                   lambda: finish(covariance()),
                   lambda: table.loglike(m, c.view(n, p * p), device.GP_FULL),
                   lambda: finish(c)])
    names = ('fused nb_gp_loglike, hyper mode', 'torch composition, hyper mode',
             'fused nb_gp_loglike, full mode', 'torch composition, full mode')
    med = [report(name, p, n, s, peak) for name, s in zip(names, stats)]
    want = finish(c)
    rel = [float(((got - want).abs() / want.abs()).max()) for got in (
        table.loglike(m, h, device.GP_HYPER),
        table.loglike(m, c.view(n, p * p), device.GP_FULL))]
    print('    torch / fused = %.2f (hyper), %.2f (full); max relative '
          'difference %.2e, %.2e' % (med[1] / med[0], med[3] / med[2], *rel),
          flush=True)


def main():
    out = os.path.join(ROOT, 'profiles', 'r07', 'gp_bench.txt')
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
