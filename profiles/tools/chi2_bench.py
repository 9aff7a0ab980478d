# Fused data-vector likelihood (nb_chi2_loglike) against the torch composition
# a user would write, ((m - d) @ W.T).square().sum(1), on the same tensors:
# time per call, the ratio torch / fused, and the fraction of the fp64 MFMA
# peak (n P (P + 16) flop) DESIGN.md section 8 uses, at (P, n) = (128, 65536),
# (512, 65536), (1024, 8192), (1024, 65536), (4096, 8192); and the diagonal
# kernel against ((m - d) / s).square().sum(1) at (1024, 65536) with its
# fraction of the HBM peak (8 P + 8 bytes per point).
# Each figure is the median (min, max) of 20 calls timed one by one with
# device events after 5 warm-up calls.  Every shape runs in a child process of
# its own under a time limit; the first one that fails ends the run.
# usage: python profiles/tools/chi2_bench.py [--out FILE]
#        (default profiles/r07/chi2_bench.txt)
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

REPEAT, WARMUP = 20, 5
PEAK_FLOPS, PEAK_BYTES = 78.6e12, 8e12
SHAPES = [(128, 65536, 'full'), (512, 65536, 'full'), (1024, 8192, 'full'),
          (1024, 65536, 'full'), (4096, 8192, 'full'), (1024, 65536, 'sigma')]
STEP_SECONDS = 240


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


def report(name, p, n, stat, flop, byts):
    med, lo, hi = stat
    print('P=%d n=%d %-34s median %9.1f us (min %9.1f, max %9.1f)  '
          '%6.2f TFLOP/s = %.3f of MFMA peak, %7.1f GB/s = %.3f of HBM peak' % (
              p, n, name, med, lo, hi, flop / (med * 1e-6) / 1e12,
              flop / (med * 1e-6) / PEAK_FLOPS, byts / (med * 1e-6) / 1e9,
              byts / (med * 1e-6) / PEAK_BYTES), flush=True)
    return med


def step(p, n, kind):
    import numpy as np
    import torch
    from nautilus_amd import device
    rng = np.random.default_rng(p + n)
    d = rng.normal(size=p)
    m = torch.from_numpy(d).cuda() + torch.randn(
        (n, p), dtype=torch.float64, device='cuda',
        generator=torch.Generator('cuda').manual_seed(p))
    d_dev = torch.from_numpy(d).cuda()
    byts = n * (8 * p + 8)
    if kind == 'sigma':
        s = 0.5 + rng.random(p)
        s_dev = torch.from_numpy(s).cuda()
        table = device.Chi2Table(d, inv_sigma=1.0 / s)
        flop = 4 * n * p
        t_new = report('fused (sigma)', p, n,
                       timed(lambda: table.loglike(m)), flop, byts)
        t_old = report('torch ((m - d) / s).square().sum(1)', p, n, timed(
            lambda: ((m - d_dev) / s_dev).square().sum(1)), flop, byts)
        want = -0.5 * ((m - d_dev) / s_dev).square().sum(1)
    else:
        # a dense lower-triangular W with a dominant diagonal
        w = np.tril(rng.normal(size=(p, p)) / np.sqrt(p)) + np.eye(p)
        w_dev = torch.from_numpy(w).cuda()
        table = device.Chi2Table(d, chol_inv=w)
        flop = n * p * (p + 16)
        t_new = report('fused', p, n, timed(lambda: table.loglike(m)), flop,
                       byts)
        t_old = report('torch ((m - d) @ W.T).square().sum(1)', p, n, timed(
            lambda: ((m - d_dev) @ w_dev.T).square().sum(1)), flop, byts)
        want = -0.5 * ((m - d_dev) @ w_dev.T).square().sum(1)
    got = table.loglike(m)
    rel = float(((got - want).abs() / want.abs()).max())
    print('    torch / fused = %.2f, max relative difference %.2e' % (
        t_old / t_new, rel), flush=True)


def main():
    out = os.path.join(ROOT, 'profiles', 'r07', 'chi2_bench.txt')
    if '--out' in sys.argv:
        out = sys.argv[sys.argv.index('--out') + 1]
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, 'w') as f:
        for p, n, kind in SHAPES:
            res = subprocess.run(
                [sys.executable, os.path.abspath(__file__), '--step', str(p),
                 str(n), kind], stdout=subprocess.PIPE,
                stderr=subprocess.STDOUT, timeout=STEP_SECONDS, text=True)
            sys.stdout.write(res.stdout)
            sys.stdout.flush()
            f.write(res.stdout)
            f.flush()
            if res.returncode != 0:
                sys.exit('step P=%d n=%d %s ended with status %d' % (
                    p, n, kind, res.returncode))


if __name__ == '__main__':
    if '--step' in sys.argv:
        i = sys.argv.index('--step')
        step(int(sys.argv[i + 1]), int(sys.argv[i + 2]), sys.argv[i + 3])
    else:
        main()
