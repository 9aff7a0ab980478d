"""Exact quantiles of the truncated normal distribution, and how far scipy's
``truncnorm.isf`` is from them, as a fixture for the device prior transform
(tests/test_prior_families_gpu.py).

For each pair (a, b) and each of 2000 points u in [1e-6, 1 - 1e-6] the value
x with  sf(x) = q,  q = fl(1 - u)  (the argument that ``Prior`` hands to
``dist.isf``, rounded once) is computed with 60-digit mpmath:

    Phi(x) = Phi(a) + (1 - q) (Phi(b) - Phi(a)),   x = sqrt(2) erfinv(2 Phi(x) - 1)

with the mirrored formula on the right of the mode, so that no argument comes
near 1.  Four more intervals lie so far out that their mass underflows in
double precision (``far_pairs``); there the equation log sf(x) = log(q sf(a) +
(1 - q) sf(b)) is solved by Newton's method in the same 60 digits.  Needs
mpmath and scipy, no GPU:

    python tests/golden/make_golden_truncnorm.py

Writes truncnorm_exact.npz: ``pairs`` (7, 2), ``u`` (2000,), ``exact``
(7, 2000) and ``scipy_dev`` (7,), the largest deviation of scipy's isf(1 - u)
from ``exact`` over the 2000 points in units of the project's band for normal
quantiles (rtol 1e-12 with atol 1e-13, i.e. |difference| / (0.1 + |exact|):
purely relative figures are meaningless where a quantile crosses zero).  Only
data is stored; ``far_pairs`` (4, 2), ``far_exact`` (4, 2000) and
``far_scipy_dev`` (4,) are the same for the far intervals."""

import os

import mpmath as mp
import numpy as np
from scipy.stats import truncnorm

HERE = os.path.dirname(os.path.abspath(__file__))
PAIRS = [(-1.0, 2.0), (2.0, 6.0), (-np.inf, 1.0), (5.0, np.inf), (-8.0, -6.0),
         (-3.0, 3.0), (0.0, np.inf)]
FAR_PAIRS = [(40.0, np.inf), (36.0, 37.0), (-np.inf, -38.0), (-101.0, -100.0)]
LO = 1e-6

mp.mp.dps = 60


def points():
    """1000 uniform points, 500 that crowd the lower end and 500 that crowd
    the upper end of [LO, 1 - LO] (log-uniform distance from the end)."""
    rng = np.random.default_rng(2024)
    flat = LO + (1 - 2 * LO) * rng.random(1000)
    low = np.exp(rng.uniform(np.log(LO), np.log(0.5), 500))
    high = 1.0 - np.exp(rng.uniform(np.log(LO), np.log(0.5), 500))
    u = np.sort(np.concatenate([flat, low, high]))
    assert u[0] >= LO and u[-1] <= 1 - LO
    return u


def _phi(x):
    """Phi(x) for x <= 0 without cancellation."""
    return mp.erfc(-x / mp.sqrt(2)) / 2


def _to_mp(v):
    return mp.mpf('-inf') if v == -np.inf else (
        mp.mpf('inf') if v == np.inf else mp.mpf(float(v)))


def exact_isf(q, a, b):
    """x with sf(x) = q for the standard normal truncated to [a, b]."""
    q, a, b = mp.mpf(float(q)), _to_mp(a), _to_mp(b)
    p = 1 - q
    # lower-tail and upper-tail probabilities of x under the full normal
    lower = q * _phi(a) + p * _phi(b) if b <= 0 else \
        q * _phi(a) + p * (1 - _phi(-b))
    upper = q * _phi(-a) + p * _phi(-b) if a >= 0 else \
        q * (1 - _phi(a)) + p * _phi(-b)
    if lower <= upper:
        return -mp.sqrt(2) * mp.erfinv(1 - 2 * lower)
    return mp.sqrt(2) * mp.erfinv(1 - 2 * upper)


def _sf(x):
    return mp.erfc(x / mp.sqrt(2)) / 2


def exact_isf_far(q, a, b):
    """The same for an interval far in one tail (mirrored to the right one):
    Newton on log sf(x) from the asymptotic solution."""
    if b < 0:
        return -exact_isf_far(1.0 - q, -b, -a)
    q, a, b = mp.mpf(float(q)), _to_mp(a), _to_mp(b)
    ratio = q + (1 - q) * (_sf(b) / _sf(a) if b != mp.inf else 0)
    if ratio == 0:
        return b
    target = mp.log(ratio) + mp.log(_sf(a))
    x = mp.sqrt(a * a - 2 * mp.log(ratio))
    for _ in range(12):
        hazard = mp.exp(-x * x / 2) / mp.sqrt(2 * mp.pi) / _sf(x)
        x += (mp.log(_sf(x)) - target) / hazard
    return x


def deviation(got, exact):
    return np.max(np.abs(got - exact) / (0.1 + np.abs(exact)))


def main():
    u = points()
    q = 1.0 - u
    exact = np.empty((len(PAIRS), len(u)))
    dev = np.empty(len(PAIRS))
    for k, (a, b) in enumerate(PAIRS):
        exact[k] = [float(exact_isf(qi, a, b)) for qi in q]
        got = truncnorm(a, b).isf(q)
        dev[k] = deviation(got, exact[k])
        print('(%g, %g): scipy within %.2e of 0.1 + |x|' % (a, b, dev[k]))
    far = np.empty((len(FAR_PAIRS), len(u)))
    far_dev = np.empty(len(FAR_PAIRS))
    for k, (a, b) in enumerate(FAR_PAIRS):
        far[k] = [float(exact_isf_far(qi, a, b)) for qi in q]
        far_dev[k] = deviation(truncnorm(a, b).isf(q), far[k])
        print('(%g, %g): scipy within %.2e of 0.1 + |x|' % (a, b, far_dev[k]))
    path = os.path.join(HERE, 'truncnorm_exact.npz')
    np.savez_compressed(path, pairs=np.array(PAIRS), u=u, exact=exact,
                        scipy_dev=dev, far_pairs=np.array(FAR_PAIRS),
                        far_exact=far, far_scipy_dev=far_dev)
    print('%s %.1f KB' % (path, os.path.getsize(path) / 1024))


if __name__ == '__main__':
    main()
