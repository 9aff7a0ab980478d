# Gaussian-process likelihood of an ordered series (nb_gps_loglike) on one GPU:
#  * time per call at n = 8192 and P = 128, 1024, 16384 for the four kernels
#    (1, 2, 3 and 2 states), with the implied bytes/s of the model matrix and
#    the cycles per step of the recursion (time * 2.4 GHz / P: at n = 8192 every
#    wavefront is resident at once, so a call lasts as long as one row);
#  * at P = 128 the ratio to the dense kernel nb_gp_loglike on the same inputs;
#  * at P = 1024 the ratio, per row, to torch.linalg.cholesky_ex +
#    solve_triangular on the dense K at n = 128 (1 GB of matrices);
#  * rows per second at P = 1024 against n, 8192 to 262144.
# Launches are timed in turn with device events around every call: 3 warm-up
# rounds, then 20 timed ones; each figure is the median (min, max) of the 20.
# One process; it stops starting new measurements after LIMIT seconds and an
# alarm ends it 60 seconds later whatever it is doing.
# usage: python profiles/tools/gps_bench.py [--out FILE]
#        (default profiles/r08/gps_bench.txt)
import os
import signal
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

REPEAT, WARMUP = 20, 3
LIMIT = 420
KERNELS = ('exp', 'matern32', 'matern52', 'sho')
HBM_PEAK = 8.0e12                            # bytes/s, MI355X data sheet
CLOCK = 2.4e9                                # Hz, the peak engine clock


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


def series(p, n, kernel, seed=0):
    import numpy as np
    import torch
    from nautilus_amd import device
    rng = np.random.default_rng([p, seed])
    t = np.sort(rng.uniform(0, 0.1 * p, size=p))
    d = rng.normal(size=p)
    s2 = (0.05 + 0.1 * rng.random(p))**2
    table = device.GPSTable(t, d, s2, kernel=kernel)
    gen = torch.Generator('cuda').manual_seed(p)
    m = torch.randn((n, p), dtype=torch.float64, device='cuda', generator=gen)
    m.add_(torch.from_numpy(d).cuda())
    h = torch.rand((n, 4), dtype=torch.float64, device='cuda', generator=gen)
    h[:, 0] += 0.5                               # a in [0.5, 1.5)
    h[:, 1] = 0.3 + 2.0 * h[:, 1]                # l in [0.3, 2.3)
    h[:, 2] = 0.01 + 0.1 * h[:, 2]               # s in [0.01, 0.11)
    h[:, 3] = 0.6 + 20.0 * h[:, 3]               # q in [0.6, 20.6)
    h = h if kernel == 'sho' else h[:, :3]
    return t, d, s2, table, m, h


def main():
    import numpy as np
    import torch
    from nautilus_amd import device
    out = os.path.join(ROOT, 'profiles', 'r08', 'gps_bench.txt')
    if '--out' in sys.argv:
        out = sys.argv[sys.argv.index('--out') + 1]
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    start = time.monotonic()
    signal.alarm(LIMIT + 60)
    f = open(out, 'w')

    def say(text):
        print(text, flush=True)
        f.write(text + '\n')
        f.flush()

    def in_time():
        return time.monotonic() - start < LIMIT

    clock = CLOCK
    say('device clock taken as %.0f MHz, HBM peak as %.1f TB/s' % (
        clock / 1e6, HBM_PEAK / 1e12))
    n = 8192
    for p in (128, 1024, 16384):
        for kernel in KERNELS:
            if not in_time():
                say('out of time')
                return
            t, d, s2, table, m, h = series(p, n, kernel)
            launches = [lambda: table.loglike(m, h)]
            names = ['nb_gps_loglike']
            if p == 128 and kernel != 'sho':
                dense = device.GPTable(d, s2, np.abs(t[:, None] - t[None, :]),
                                       kernel=kernel)
                launches.append(lambda: dense.loglike(m, h, device.GP_HYPER))
                names.append('nb_gp_loglike')
            stats = timed(launches)
            med = stats[0][0]
            say('P=%d n=%d %-9s nb_gps_loglike median %10.1f us (min %10.1f, '
                'max %10.1f)  %7.1f GB/s of m = %.4f of the HBM peak, %6.1f '
                'cycles per step' % (p, n, kernel, *stats[0],
                                     n * p * 8 / (med * 1e-6) / 1e9,
                                     n * p * 8 / (med * 1e-6) / HBM_PEAK,
                                     med * 1e-6 * clock / p))
            if len(stats) > 1:
                a, b = table.loglike(m, h), dense.loglike(m, h,
                                                          device.GP_HYPER)
                say('    nb_gp_loglike median %10.1f us (min %10.1f, max '
                    '%10.1f): dense / filter = %.2f; max relative difference '
                    '%.2e' % (*stats[1], stats[1][0] / med,
                              float(((a - b).abs() / b.abs()).max())))
            del table, m, h
    # P = 1024 against the dense route of torch, per row
    p, n_dense = 1024, 128
    if in_time():
        t, d, s2, table, m, h = series(p, n_dense, 'matern32')
        dist = torch.from_numpy(np.abs(t[:, None] - t[None, :])).cuda()
        d_dev, s2_dev = torch.from_numpy(d).cuda(), torch.from_numpy(s2).cuda()
        eye = torch.eye(p, dtype=torch.float64, device='cuda')

        def dense_route():
            u = 3.0**0.5 * dist / h[:, 1, None, None]
            k = h[:, 0, None, None] * (1 + u) * torch.exp(-u) + \
                (h[:, 2, None, None] + s2_dev[None, :, None]) * eye
            chol, _ = torch.linalg.cholesky_ex(k)
            y = torch.linalg.solve_triangular(chol, (m - d_dev).unsqueeze(2),
                                              upper=False)
            log_det = 2 * torch.log(torch.diagonal(chol, dim1=1, dim2=2)).sum(1)
            return -0.5 * ((y * y).sum((1, 2)) + log_det)

        stats = timed([lambda: table.loglike(m, h), dense_route])
        a, b = table.loglike(m, h), dense_route()
        say('P=%d n=%d matern32 nb_gps_loglike median %10.1f us; torch '
            'cholesky_ex + solve_triangular median %10.1f us (min %10.1f, '
            'max %10.1f): torch / filter = %.1f at this n; max relative '
            'difference %.2e' % (p, n_dense, stats[0][0], *stats[1],
                                 stats[1][0] / stats[0][0],
                                 float(((a - b).abs() / b.abs()).max())))
        big = series(p, 8192, 'matern32')
        med = timed([lambda: big[3].loglike(big[4], big[5])])[0][0]
        say('    per row: torch %.2f us, filter at n = 8192 %.4f us: ratio '
            '%.0f' % (stats[1][0] / n_dense, med / 8192,
                      stats[1][0] / n_dense / (med / 8192)))
        del table, m, h, dist, big
    # throughput against n
    for kernel in ('exp', 'matern32', 'matern52'):
        for n in (8192, 32768, 131072, 262144):
            if not in_time():
                say('out of time')
                return
            t, d, s2, table, m, h = series(1024, n, kernel)
            med, lo, hi = timed([lambda: table.loglike(m, h)])[0]
            say('P=1024 n=%d %-9s median %10.1f us (min %10.1f, max %10.1f) '
                '%8.2f Mrows/s, %7.1f GB/s of m = %.4f of the HBM peak' % (
                    n, kernel, med, lo, hi, n / med,
                    n * 1024 * 8 / (med * 1e-6) / 1e9,
                    n * 1024 * 8 / (med * 1e-6) / HBM_PEAK))
            del table, m, h
    say('done in %.0f s' % (time.monotonic() - start))


if __name__ == '__main__':
    main()
