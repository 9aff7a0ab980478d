# Prior transform on the device: the by-value kernel behind nb_prior_transform
# (uniform / normal only) against the table-driven one in both layouts, a
# prior that cycles through all six kinds, and a plain device copy of the same
# bytes.  Each figure is the median (min, max) of 50 launches timed one by one
# with device events after a warm-up; (a) is measured twice, before and after
# (b), so that its own run-to-run spread is on the page.
# usage: python profiles/tools/prior_bench.py [rows ...]     (default 65536 4194304)
import ctypes as C
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import numpy as np
import torch
from scipy import stats
from nautilus_amd import Prior, _lib, device

D, REPEAT, WARMUP = 50, 50, 5
lib = _lib.load()


def timed(launch):
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


def prior_of(kinds):
    make = dict(
        uniform=lambda j: stats.uniform(loc=-3.0 + 0.37 * j, scale=1.0 + j % 7),
        norm=lambda j: stats.norm(loc=2.0 - 0.1 * j, scale=0.5 + 0.01 * j),
        loguniform=lambda j: stats.loguniform(1e-3, 10.0),
        lognorm=lambda j: stats.lognorm(0.7),
        halfnorm=lambda j: stats.halfnorm(scale=1.0 + 0.1 * j),
        truncnorm=lambda j: stats.truncnorm(-1.0, 2.0))
    prior = Prior()
    for j in range(D):
        prior.add_parameter('p%d' % j, dist=make[kinds[j % len(kinds)]](j))
    return prior


def old_launch(prior, u, out):
    kind, loc, scale = prior.device_spec()
    args = (device._ptr(u), u.shape[0], D, kind.ctypes.data_as(C.c_void_p),
            device._dp(loc), device._dp(scale), device._ptr(out))
    keep = (kind, loc, scale)

    def launch():
        _lib.check(lib.nb_prior_transform(*args, device._stream()))
    launch.keep = keep
    return launch


def new_launch(prior, u, out, layout):
    handle = prior._device_handle()

    def launch():
        _lib.check(lib.nb_prior_table_transform(
            handle._h, device._ptr(u), u.shape[0], layout, device._ptr(out),
            device._stream()))
    return launch


def report(name, n, stat, copy_us=None):
    med, lo, hi = stat
    gbs = 2 * 8 * n * D / med / 1e3
    line = 'n=%d d=%d %-34s median %9.1f us (min %9.1f, max %9.1f)  %7.1f GB/s' % (
        n, D, name, med, lo, hi, gbs)
    if copy_us is not None:
        line += '  copy/this = %.3f' % (copy_us / med)
    print(line, flush=True)


for n in [int(v) for v in sys.argv[1:]] or [65536, 1 << 22]:
    u = torch.rand((n, D), dtype=torch.float64, device='cuda')
    out = torch.empty_like(u)
    out_t = torch.empty((D, n), dtype=torch.float64, device='cuda')
    copy = timed(lambda: out.copy_(u))
    report('(d) device copy', n, copy)
    for kinds in (['uniform'], ['norm']):
        prior = prior_of(kinds)
        old = old_launch(prior, u, out)
        a1 = timed(old)
        ref = out.clone()
        b_row = timed(new_launch(prior, u, out, device.ROW_MAJOR))
        diff = float((out - ref).abs().max())
        b_col = timed(new_launch(prior, u, out_t, device.COLUMN_MAJOR))
        same = bool(torch.equal(out_t.t(), out))
        a2 = timed(old)
        report('(a) nb_prior_transform %s' % kinds[0], n, a1, copy[0])
        report('(a) again', n, a2, copy[0])
        report('(b) table, row-major %s' % kinds[0], n, b_row, copy[0])
        report('(b) table, column-major %s' % kinds[0], n, b_col, copy[0])
        print('    max |new - old| = %.3e, column-major == row-major^T: %s' % (
            diff, same), flush=True)
    prior = prior_of(['uniform', 'norm', 'loguniform', 'lognorm', 'halfnorm',
                      'truncnorm'])
    report('(c) six kinds, row-major', n,
           timed(new_launch(prior, u, out, device.ROW_MAJOR)), copy[0])
    report('(c) six kinds, column-major', n,
           timed(new_launch(prior, u, out_t, device.COLUMN_MAJOR)), copy[0])
