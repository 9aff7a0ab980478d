# Gaussian-process likelihood of an ordered series with a SUM of kernel terms
# (nb_gps_create_terms / nb_gps_loglike, nb_gps_filter.h) on one GPU, next to
# gps_bench.py:
#  * time per call at n = 8192 and P = 128, 1024, 16384 for composite kernels
#    and, in the same run, for the single-term 'matern52' and 'sho', with the
#    cycles per step of the recursion (time * 2.4 GHz / P: at n = 8192 every
#    wavefront is resident at once, so a call lasts as long as one row);
#  * at P = 128 the ratio to what a user had before: the same K built in torch
#    as an (n, P, P) tensor (1 GB) and GaussianProcessLikelihood(cov='full')'s
#    kernel nb_gp_loglike on it; the build and the launch are timed apart.
# Launches are timed in turn with device events around every call: 3 warm-up
# rounds, then 20 timed ones; each figure is the median (min, max) of the 20.
# One process; it stops starting new measurements after LIMIT seconds and an
# alarm ends it 60 seconds later whatever it is doing.
# usage: python profiles/tools/gps_terms_bench.py [--out FILE] [--quick]
#        (default profiles/gps_terms/gps_terms_bench.txt; --quick: P = 1024
#        only)
import os
import signal
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from gps_bench import CLOCK, timed  # noqa: E402

LIMIT = 300
KERNELS = ('matern52', 'sho', ('exp', 'exp'), ('exp', 'sho'), ('sho', 'sho'),
           ('matern52', 'matern52'), ('exp', 'matern32', 'matern52'),
           ('sho', 'sho', 'sho'))


def name_of(kernel):
    return kernel if isinstance(kernel, str) else '+'.join(kernel)


def series(p, n, kernel, seed=0):
    """The series of gps_bench.py; per term a in [0.5, 1.5), l in [0.3, 2.3)
    and q in [0.6, 20.6), s in [0.01, 0.11)."""
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
    h = torch.rand((n, table.width), dtype=torch.float64, device='cuda',
                   generator=gen)
    if isinstance(kernel, str):
        h[:, 0] += 0.5
        h[:, 1] = 0.3 + 2.0 * h[:, 1]
        h[:, 2] = 0.01 + 0.1 * h[:, 2]
        if kernel == 'sho':
            h[:, 3] = 0.6 + 20.0 * h[:, 3]
        return t, d, s2, table, m, h
    col = 0
    for name in kernel:
        h[:, col] += 0.5
        h[:, col + 1] = 0.3 + 2.0 * h[:, col + 1]
        if name == 'sho':
            h[:, col + 2] = 0.6 + 20.0 * h[:, col + 2]
        col += 3 if name == 'sho' else 2
    h[:, col] = 0.01 + 0.1 * h[:, col]
    return t, d, s2, table, m, h


def rho(name, r, q=None):
    import torch
    if name == 'exp':
        return torch.exp(-r)
    if name == 'matern32':
        x = 3.0**0.5 * r
        return (1 + x) * torch.exp(-x)
    if name == 'matern52':
        x = 5.0**0.5 * r
        return (1 + x + x * x / 3) * torch.exp(-x)
    w = 1 / (2 * q)
    eta = torch.sqrt(1 - w * w)
    return torch.exp(-r * w) * (torch.cos(eta * r) + torch.sin(eta * r) / eta * w)


def covariance(kernel, dist, h):
    """sum_i a_i rho_i(dist / l_i) + s I as an (n, P, P) tensor."""
    import torch
    col, k = 0, None
    for name in kernel:
        a, l = h[:, col, None, None], h[:, col + 1, None, None]
        q = h[:, col + 2, None, None] if name == 'sho' else None
        term = a * rho(name, dist / l, q)
        k = term if k is None else k.add_(term)
        del term
        col += 3 if name == 'sho' else 2
    k.diagonal(dim1=1, dim2=2).add_(h[:, col, None])
    return k


def main():
    import numpy as np
    import torch
    from nautilus_amd import device
    out = os.path.join(ROOT, 'profiles', 'gps_terms', 'gps_terms_bench.txt')
    if '--out' in sys.argv:
        out = sys.argv[sys.argv.index('--out') + 1]
    sizes = (1024,) if '--quick' in sys.argv else (128, 1024, 16384)
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    start = time.monotonic()
    signal.alarm(LIMIT + 60)
    f = open(out, 'w')

    def say(text):
        print(text, flush=True)
        f.write(text + '\n')
        f.flush()

    say('device clock taken as %.0f MHz' % (CLOCK / 1e6))
    n = 8192
    for p in sizes:
        single = {}
        for kernel in KERNELS:
            if time.monotonic() - start > LIMIT:
                say('out of time')
                return
            t, d, s2, table, m, h = series(p, n, kernel)
            med, lo, hi = timed([lambda: table.loglike(m, h)])[0]
            cycles = med * 1e-6 * CLOCK / p
            text = 'P=%d n=%d %-24s median %10.1f us (min %10.1f, max ' \
                '%10.1f) %7.1f cycles per step' % (p, n, name_of(kernel),
                                                   med, lo, hi, cycles)
            if isinstance(kernel, str):
                single[kernel] = cycles
            else:
                text += '; over matern52 %.2f, over sho %.2f' % (
                    cycles / single['matern52'], cycles / single['sho'])
            say(text)
            if p == 128 and not isinstance(kernel, str):
                dist = torch.from_numpy(np.abs(t[:, None] - t[None, :])).cuda()
                dense = device.GPTable(d, s2)
                k = covariance(kernel, dist, h)
                build, launch = timed([
                    lambda: covariance(kernel, dist, h),
                    lambda: dense.loglike(m, k, device.GP_FULL)])
                a, b = table.loglike(m, h), dense.loglike(m, k, device.GP_FULL)
                say('    K in torch median %10.1f us, nb_gp_loglike (full) '
                    'median %10.1f us: (build + dense) / filter = %.1f, dense '
                    '/ filter = %.1f; max relative difference %.2e' % (
                        build[0], launch[0], (build[0] + launch[0]) / med,
                        launch[0] / med,
                        float(((a - b).abs() / b.abs()).max())))
                del dist, dense, k
            del table, m, h
    say('done in %.0f s' % (time.monotonic() - start))


if __name__ == '__main__':
    main()
