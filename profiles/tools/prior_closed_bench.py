# The closed-form tier of the device prior transform (kinds 7 to 17) against
# the all-loguniform table (kind 2, the level-0 kernel) at the same shape, in
# one process: d = 50, both layouts.  The tables take turns for ROUNDS rounds of
# REPEAT launches, each launch timed on its own with device events after a
# warm-up; a figure is the median (min, max) of a table's ROUNDS x REPEAT
# launches.  Then every closed-form kind alone (50 columns of it, row-major),
# to show which of them the mixed table's time comes from.
# usage: python profiles/tools/prior_closed_bench.py [rows ...]   (default 65536)
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import numpy as np
import torch
from scipy import stats
from nautilus_amd import Prior, _lib, device

D, REPEAT, ROUNDS, WARMUP = 50, 10, 5, 5
lib = _lib.load()

MAKE = dict(
    loguniform=lambda j: stats.loguniform(1e-3, 10.0),
    cauchy=lambda j: stats.cauchy(loc=0.1 * j, scale=2.0),
    halfcauchy=lambda j: stats.halfcauchy(scale=1.0 + 0.1 * j),
    laplace=lambda j: stats.laplace(loc=-1.0, scale=0.5),
    logistic=lambda j: stats.logistic(loc=2.0, scale=0.5),
    gumbel_r=lambda j: stats.gumbel_r(loc=0.5, scale=1.5),
    gumbel_l=lambda j: stats.gumbel_l(scale=4.0),
    weibull_min=lambda j: stats.weibull_min(2.5, scale=2.0),
    rayleigh=lambda j: stats.rayleigh(scale=0.75),
    pareto=lambda j: stats.pareto(3.0, scale=2.0),
    powerlaw=lambda j: stats.powerlaw(3.5, scale=4.0),
    triang=lambda j: stats.triang(0.3, loc=-1.0, scale=2.0))
CLOSED = [k for k in MAKE if k != 'loguniform']


def prior_of(kinds):
    prior = Prior()
    for j in range(D):
        prior.add_parameter('p%d' % j, dist=MAKE[kinds[j % len(kinds)]](j))
    return prior


def launcher(prior, u, out, layout):
    handle = prior._device_handle()

    def launch():
        _lib.check(lib.nb_prior_table_transform(
            handle._h, device._ptr(u), u.shape[0], layout, device._ptr(out),
            device._stream()))
    launch.keep = prior
    return launch


def one_by_one(launch, repeat):
    us = []
    for _ in range(repeat):
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        ev[0].record()
        launch()
        ev[1].record()
        ev[1].synchronize()
        us.append(ev[0].elapsed_time(ev[1]) * 1e3)
    return us


def alternate(launches):
    """name -> (median, min, max) in microseconds, the tables taking turns"""
    for launch in launches.values():
        for _ in range(WARMUP):
            launch()
    torch.cuda.synchronize()
    us = {name: [] for name in launches}
    for _ in range(ROUNDS):
        for name, launch in launches.items():
            us[name] += one_by_one(launch, REPEAT)
    return {name: (np.median(v), min(v), max(v)) for name, v in us.items()}


def report(n, name, stat):
    print('n=%d d=%d %-36s median %8.1f us (min %8.1f, max %8.1f)' % (
        (n, D, name) + stat), flush=True)


for n in [int(v) for v in sys.argv[1:]] or [65536]:
    u = torch.rand((n, D), dtype=torch.float64, device='cuda')
    out = torch.empty_like(u)
    out_t = torch.empty((D, n), dtype=torch.float64, device='cuda')
    closed, flat = prior_of(CLOSED), prior_of(['loguniform'])
    stat = alternate({
        'copy': lambda: out.copy_(u),
        'loguniform, row-major': launcher(flat, u, out, device.ROW_MAJOR),
        'eleven closed-form kinds, row-major':
            launcher(closed, u, out, device.ROW_MAJOR),
        'loguniform, column-major':
            launcher(flat, u, out_t, device.COLUMN_MAJOR),
        'eleven closed-form kinds, column-major':
            launcher(closed, u, out_t, device.COLUMN_MAJOR)})
    for name, s in stat.items():
        report(n, name, s)
    for layout in ('row-major', 'column-major'):
        print('n=%d closed-form / loguniform, %s: %.2f' % (
            n, layout, stat['eleven closed-form kinds, ' + layout][0] /
            stat['loguniform, ' + layout][0]), flush=True)
    want = closed.unit_to_physical(u[:64].cpu().numpy())
    got = closed.unit_to_physical(u[:64]).cpu().numpy()
    print('n=%d closed-form table against scipy on 64 rows: max relative '
          'difference %.2e' % (n, np.max(np.abs(got - want) / np.abs(want))),
          flush=True)
    singles = {kind: launcher(prior_of([kind]), u, out, device.ROW_MAJOR)
               for kind in ['loguniform'] + CLOSED}
    for name, s in alternate(singles).items():
        report(n, '%s alone, row-major' % name, s)
