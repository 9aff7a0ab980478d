"""Exact quantiles of the eleven closed-form families of the device prior
transform (kinds 7 to 17), and how far scipy's ``isf`` is from them, as a
fixture for tests/test_prior_closed_form.py and
tests/test_prior_closed_form_gpu.py.

For each family (and shape) and each of 1005 points u the value x with
sf(x) = q,  q = fl(1 - u)  (the argument that ``Prior`` hands to ``dist.isf``,
rounded once) is computed with 60-digit mpmath from the quantile function of
the standard distribution; the shape is the double that scipy is given, not a
rounded reciprocal of it.  The points: 500 that crowd the lower end of
[1e-6, 1 - 1e-6] geometrically (a constant ratio from 1e-6 to 1/2), their
mirror images 1 - u that crowd the upper end, and 0.25, 0.5, 0.75, e^-1 and
1 - e^-1 -- the medians, the points where the formulas change sides and the
zero of both Gumbel quantiles.  Needs mpmath and scipy, no GPU:

    python tests/golden/make_golden_quantiles.py

Writes quantile_exact.npz: ``u`` (1005,), sorted; ``names`` (22,), scipy's
name of the family of each row; ``shapes`` (22,), its shape or nan; ``exact``
(22, 1005); ``scipy_dev`` (22,), the largest |scipy's isf(1 - u) - exact| /
(1e-13 + 1e-12 |exact|) over the points -- the project's band for quantiles
(rtol 1e-12, atol 1e-13) as the unit.  Only data is stored."""

import os

import mpmath as mp
import numpy as np
from scipy import stats

HERE = os.path.dirname(os.path.abspath(__file__))
LO = 1e-6
CASES = [('cauchy', None), ('halfcauchy', None), ('laplace', None),
         ('logistic', None), ('gumbel_r', None), ('gumbel_l', None)] + \
    [('weibull_min', c) for c in (0.3, 1.0, 2.5, 8.0)] + \
    [('rayleigh', None)] + \
    [('pareto', b) for b in (0.5, 1.0, 3.0, 20.0)] + \
    [('powerlaw', a) for a in (0.2, 1.0, 3.5)] + \
    [('triang', c) for c in (0.0, 0.3, 0.5, 1.0)]

mp.mp.dps = 60


def points():
    low = np.geomspace(LO, 0.5, 501)[:-1]
    low[0] = LO
    special = [0.25, 0.5, 0.75, np.exp(-1.0), 1.0 - np.exp(-1.0)]
    u = np.unique(np.concatenate([low, 1.0 - low, special]))
    assert u.size == 1005 and u[0] == LO and u[-1] == 1.0 - LO
    return u


def exact_isf(name, shape, q):
    """x with sf(x) = q for the standard distribution, q a double."""
    q = mp.mpf(float(q))
    p = 1 - q
    s = None if shape is None else mp.mpf(float(shape))
    if name == 'cauchy':
        return mp.cot(mp.pi * q)
    if name == 'halfcauchy':
        return mp.cot(mp.pi * q / 2)
    if name == 'laplace':
        return -mp.log(2 * q) if q <= mp.mpf(1) / 2 else mp.log(2 * p)
    if name == 'logistic':
        return mp.log(p / q)
    if name == 'gumbel_r':
        return -mp.log(-mp.log(p))
    if name == 'gumbel_l':
        return mp.log(-mp.log(q))
    if name == 'weibull_min':
        return (-mp.log(q))**(1 / s)
    if name == 'rayleigh':
        return mp.sqrt(-2 * mp.log(q))
    if name == 'pareto':
        return q**(-1 / s)
    if name == 'powerlaw':
        return p**(1 / s)
    assert name == 'triang'
    return mp.sqrt(s * p) if p < s else 1 - mp.sqrt((1 - s) * q)


def main():
    u = points()
    q = 1.0 - u
    exact = np.empty((len(CASES), len(u)))
    dev = np.empty(len(CASES))
    for k, (name, shape) in enumerate(CASES):
        exact[k] = [float(exact_isf(name, shape, qi)) for qi in q]
        dist = getattr(stats, name)(*([] if shape is None else [shape]))
        dev[k] = np.max(np.abs(dist.isf(q) - exact[k]) /
                        (1e-13 + 1e-12 * np.abs(exact[k])))
        print('%s %s: scipy within %.2e of the band' % (name, shape, dev[k]))
    path = os.path.join(HERE, 'quantile_exact.npz')
    np.savez_compressed(
        path, u=u, names=np.array([n for n, _ in CASES]),
        shapes=np.array([np.nan if s is None else s for _, s in CASES]),
        exact=exact, scipy_dev=dev)
    print('%s %.1f KB' % (path, os.path.getsize(path) / 1024))


if __name__ == '__main__':
    main()
