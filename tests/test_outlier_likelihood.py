"""Host side of ``GaussianOutlierLikelihood``: the numpy twin against scipy,
``GaussianNoiseLikelihood`` and ``np.longdouble``, the responsibilities, the
NaN rules, constructor validation and pickling; and the problems, the
reference and the error budget that test_outlier_likelihood_gpu.py holds the
device kernel to."""

import functools
import math
import pickle

import numpy as np
import pytest
import torch

from nautilus_amd import GaussianNoiseLikelihood, GaussianOutlierLikelihood
from test_noise_likelihood import budget as noise_budget
from test_noise_likelihood import reference as noise_reference

EPS = 2.0**-52
P_TOP = 1.0 - 2.0**-53             # the largest p below 1
FAR = 745.0                        # exp(-745) is below the smallest double

# every P and every n of the two lists appears; the kernel changes its shape
# (L, R, U) after P = 32 and after P = 512 (device.outlier_launch_shape; the
# GPU file finds the boundaries from the function)
P_ALL = (1, 3, 15, 16, 17, 32, 33, 63, 64, 65, 512, 513, 4099)
N_ALL = (1, 15, 17, 1000, 4097)
# (P, n, rot): a column's class is (j + rot) % 4, see problem().  From P = 15
# on a case holds every class and every kind of element, which takes rows of
# every p class: n >= 15; P = 1 and P = 3 cannot, run once per rot instead and
# take n = 1 among theirs.  The order of the long P keeps n P below 4.3
# million.
_P_LONG = (15, 16, 17, 32, 33, 63, 64, 65, 4099, 512, 513)
SHAPES = [(p, N_ALL[1 + (i + s) % 4], 0) for i, p in enumerate(_P_LONG)
          for s in (0, 2)] + \
    [(p, N_ALL[(rot + p + 3) % 5], rot) for p in (1, 3) for rot in range(4)]
assert {s[0] for s in SHAPES} == set(P_ALL)
assert {s[1] for s in SHAPES} == set(N_ALL)
assert max(s[0] * s[1] for s in SHAPES) < 4.3e6
# a row whose running products must be renormalised: every B in [1, 1.001) has
# a mantissa near 1/2, and at P = 131075 a lane of a wavefront-wide row sees
# 2049 elements, 513 per product, two renormalisations
LONG_SHAPE = (131075, 33)
# what the bit-for-bit and the edge tests of the GPU file read: one P on each
# launch shape
ROW_TEST_P = (3, 129, 1025)
EDGE_TEST_P = (17, 129, 1025)


def identity(x):
    return x


@functools.lru_cache(maxsize=4)
def problem(p, n, rot=0):
    """Data, sigma, n model rows and their mixture coefficients.  Column j is
    of class (j + rot) % 4, the classes of test_noise_likelihood.problem:
      0  sigma_j = 0;
      1  sigma_j^2 log-uniform in [1e-12, 1e12];
      2  sigma_j^2 in [1, 1.001);
      3  sigma_j^2 log-uniform in [0.01, 100], and m = d exactly in every
         third row.
    Row i is of class i % 5 by its outlier fraction:
      0  p = 0;  1  p = 1;  2  p = 1e-12;  3  p = 1 - 2^-53;
      4  p log-uniform in [1e-3, 0.5];
    c in [1/2, 2), a log-uniform in [1e-3, 10], f log-uniform in [1e-6, 1e-4]
    (all positive: no v cancels), b = 2 N(0, 1) and s log-uniform in [1, 100],
    but every row with i % 7 = 3 has a narrow outlier component far away, (b,
    s) = (300, 0.01), which puts the outlier exponent of its columns of
    classes 0 and 2 below -40000.
    m = d + sqrt(v(d)) N(0, 1), residuals of the size of the error bars, but:
      (i + j) % 5 = 0  m lies 50 sqrt(v(m)) from d: the inlier exponent is
                       -1250, below -745;
      (i + j) % 5 = 2  (not in the far rows) m is where the inlier exponent
                       equals the outlier one but for the rounding of m;
    both solved from the quadratic (m - d)^2 = K (c sigma^2 + a + f m^2).
    Nobody writes to the result."""
    rng = np.random.default_rng(7000003 * rot + 1000 * p + n)
    cls = (np.arange(p) + rot) % 4
    s2 = 10.0**rng.uniform(-2, 2, size=p)
    s2[cls == 0] = 0.0
    k = int(np.sum(cls == 1))                   # one per stratum of the range
    s2[cls == 1] = 10.0**(rng.permutation(
        (np.arange(k) + rng.random(k)) / max(k, 1)) * 24 - 12)
    s2[cls == 2] = (1.00001 + 0.00098 * rng.random(p))[cls == 2]
    sigma = np.sqrt(s2)
    s2 = sigma * sigma                          # what the likelihood uses
    d = (0.25 + rng.exponential(size=p)) * rng.choice([-1.0, 1.0], size=p)
    rows = np.arange(n)
    rcl = rows % 5
    pp = 10.0**rng.uniform(-3, np.log10(0.5), size=n)
    pp[rcl == 0] = 0.0
    pp[rcl == 1] = 1.0
    pp[rcl == 2] = 1e-12
    pp[rcl == 3] = P_TOP
    c = 0.5 + 1.5 * rng.random(n)
    a = 10.0**rng.uniform(-3, 1, size=n)
    f = 10.0**rng.uniform(-6, -4, size=n)
    far = rows % 7 == 3
    b = 2.0 * rng.normal(size=n)
    s = 10.0**rng.uniform(0, 2, size=n)
    b[far], s[far] = 300.0, 0.01
    base = c[:, None] * s2 + a[:, None]
    fc = f[:, None]
    m = d + np.sqrt(base + fc * d * d) * rng.normal(size=(n, p))
    slot = (rows[:, None] + np.arange(p)) % 5
    sign = rng.choice([-1.0, 1.0], size=(n, p))
    k_equal = (d - b[:, None])**2 / (s2 + s[:, None])       # -2 e2
    for where, kk in ((slot == 0, 2500.0),
                      ((slot == 2) & ~far[:, None], k_equal)):
        kk = np.broadcast_to(kk, (n, p))
        assert np.all(kk[where] * np.broadcast_to(fc, (n, p))[where] < 0.5)
        kk = np.where(where, kk, 0.0)
        root = np.sqrt(kk * fc * d * d + (1 - kk * fc) * kk * base)
        m = np.where(where, (d + sign * root) / (1 - kk * fc), m)
    exact = (rows % 3 == 0)[:, None] & (cls == 3)
    m = np.where(exact, d, m)
    w = np.stack([c, a, f, pp, b, s], axis=1)
    for arr in (d, sigma, m, w):
        arr.setflags(write=False)
    return d, sigma, m, w


def long_problem(p, n):
    """Every B in [1, 1.001): sigma^2 in (0.999, 0.9995), c = 1, a below 4e-4
    and f = 0 put v^-1/2 into (1.00005, 1.0005), p is 0, 1e-6 or 1e-5, and the
    inlier component is the larger one everywhere: residuals of a tenth of
    the error bars, the outlier mean ten away."""
    rng = np.random.default_rng(p + n)
    sigma = np.sqrt(0.99901 + 0.00048 * rng.random(p))
    d = rng.normal(size=p)
    w = np.stack([np.ones(n), 4e-4 * rng.random(n), np.zeros(n),
                  np.array([0.0, 1e-6, 1e-5])[np.arange(n) % 3],
                  10.0 + rng.normal(size=n), 1.0 + rng.random(n)], axis=1)
    m = d + 0.1 * rng.normal(size=(n, p))
    return d, sigma, m, w


def reference(d, sigma, m, w):
    """The defining formula in ``np.longdouble`` from the float64 inputs, as
    ``logaddexp`` of the two weighted log densities: log L without the
    constant, rounded once; per row X = sum_j |e_hi|, A = sum_j |log B| and
    Y = sum_j rho (|e1| + |e2|), where hi is the component with the larger
    exponent among those with a non-zero weight, B = A_hi + A_lo exp(e_lo -
    e_hi) and rho the share of its second term; and what the case holds: the
    number of elements of every kind, and the extremes of v, u and B."""
    ld = np.longdouble
    s2 = sigma.astype(ld)**2
    ml, dl = m.astype(ld), d.astype(ld)
    c, a, f, p, b, s = (w[:, i:i + 1].astype(ld) for i in range(6))
    v = c * s2 + a + f * ml * ml
    u = s2 + s
    e1 = -(ml - dl)**2 / (2 * v)
    e2 = -(dl - b)**2 / (2 * u)
    with np.errstate(divide='ignore'):
        l1 = e1 + (np.log(1 - p) - 0.5 * np.log(v))
        l2 = e2 + (np.log(p) - 0.5 * np.log(u))
    lq = np.logaddexp(l1, l2)
    has1, has2 = np.broadcast_to(p < 1, v.shape), np.broadcast_to(p > 0,
                                                                   v.shape)
    one = ~has2 | (has1 & (e1 >= e2))
    e_hi = np.where(one, e1, e2)
    log_b = lq - e_hi
    both = has1 & has2
    rho = np.where(both, np.exp(np.where(both, np.where(one, l2, l1) - lq,
                                         0)), 0)
    y = rho * (np.abs(e1) + np.abs(e2))
    b_all = np.exp(log_b)
    kinds = dict(
        inlier_far=int(np.sum((e1 < -FAR) & (e2 > -FAR))),
        both_far=int(np.sum((e1 < -FAR) & (e2 < -FAR))),
        equal=int(np.sum(both & (np.abs(e1 - e2) < 1e-3))),
        p0_outlier_larger=int(np.sum(~has2 & (e2 > e1))),
        p1_inlier_larger=int(np.sum(~has1 & (e1 > e2))),
        v_min=float(v.min()), v_max=float(v.max()),
        u_min=float(u.min()), u_max=float(u.max()),
        b_min=float(b_all.min()), b_max=float(b_all.max()))
    return lq.sum(axis=1).astype(float), \
        np.abs(e_hi).sum(axis=1).astype(float), \
        np.abs(log_b).sum(axis=1).astype(float), \
        y.sum(axis=1).astype(float), kinds


@functools.lru_cache(maxsize=None)
def expected(p, n, rot=0):
    """``reference`` of ``problem(p, n, rot)``: rows only, computed once and
    shared by both test files."""
    return reference(*problem(p, n, rot))


@functools.lru_cache(maxsize=None)
def long_expected():
    return reference(*long_problem(*LONG_SHAPE))


def budget(p, x, a, y):
    """The bound on |log L_device - log L_true| of a row, a function of the
    inputs only:

        tol = eps (6 X + A + 7 Y + 7 P) + 1/2 eps (T + 2) (X + A),

    X = sum_j |e_hi|, A = sum_j |log B|, Y = sum_j rho (|e1| + |e2|) from the
    reference, eps = 2^-52 (every rounding errs by at most eps / 2 of its
    result), log L = sum_j (e_hi + log B), B = A_hi + A_lo exp(e_lo - e_hi),
    rho = A_lo exp(e_lo - e_hi) / B.  (log q = e_hi + log B is an identity
    whichever component is called hi: where the rounded exponents order the
    two the other way than the true ones, they differ by no more than their
    errors and X, A, Y move by as little.)

    Per element.  v: sigma^2 is rounded on the host (1/2 eps of c sigma^2),
    m^2 (1/2), the inner fma (1/2 of c sigma^2 + a) and the outer one (1/2 of
    v); all terms are >= 0, so v errs by at most 3/2 eps v; u = sigma^2 + s by
    eps u.  y = v^-1/2: 3/4 from v; the second Newton step leaves 1/4 (the
    rounding of v y inside the correction), 1/2 (its last fma) and 3/2 (3/2
    e^2)^2 < 0.21 for an estimate within e = 2^-14: y errs by 7/4 eps (the
    twin's 1 / sqrt: two roundings, the same 1), u^-1/2 by 3/2.  An
    exponent: r = m - d (1/2, so r^2 carries 1), r r (1/2), y y (7/2 + 1/2),
    the product (1/2), the factor -1/2 is exact: e errs by 6 eps |e|, for e2
    less.  sum_j e_hi: 6 eps X.
    A1 = (1 - p) y: the subtraction (1/2), y (7/4), the product (1/2); A2 less:
    an amplitude errs by 3 eps.  The argument of the exp is e_lo - e_hi: 6 eps
    (|e1| + |e2|) from the exponents and 1/2 eps of itself, <= 13/2 eps (|e1|
    + |e2|), absolutely, which the exp turns into a relative error of its
    value; the exp itself within 1 ulp (the device library's documented
    bound, and glibc's), eps.  B by one fma (1/2): its relative error is at
    most 3 + 1/2 + rho (1 + 13/2 (|e1| + |e2|)) eps, and that is the absolute
    error of log B: (9/2) eps P + (13/2) eps Y.  B's mantissa enters a product
    by one multiplication (1/2 eps in its log); moving the product's exponent
    to the integer sum is exact.
    Per product (L U of them per row).  One po_log of a number in (2^-257, 1],
    within 1 ulp: eps |lg| with |lg| <= log 2 times the elements multiplied
    since the last renormalisation, <= 0.7 eps P over the row.  The integer
    exponent E times the double nearest log 2, joined by one fma: 1/2 eps E
    log 2 for the constant and 1/2 eps of the result, a partial sum of the log
    B; with |E log 2| <= |partial sum| + |lg| that is eps A + 0.35 eps P.
    Together (9/2 + 1/2 + 0.7 + 0.35) eps P <= 7 eps P, 13/2 eps Y <= 7 eps Y
    and eps A.
    Sums.  A row's partial sum of the e_hi takes one addition per step, ceil(P
    / (L U)) of them, then one to join the log, log2(U) in the tree, log2(L)
    across the lanes and one for the constant: T + 2 additions, T = ceil(P /
    (L U)) + log2(L U), each erring by eps / 2 of a partial sum that is at
    most X + A in size.  T is capped at P / 16 + 8."""
    from nautilus_amd import device
    lanes, _, u = device.outlier_launch_shape(p)
    t = min(math.ceil(p / (lanes * u)) + math.log2(lanes * u), p / 16 + 8)
    return EPS * (6 * x + a + 7 * y + 7 * p) + 0.5 * EPS * (t + 2) * (x + a)


def make(d, sigma, normalised=False):
    return GaussianOutlierLikelihood(identity, d, sigma,
                                     normalised=normalised)


def check_classes(p, n, rot):
    """What a case of ``problem`` holds, checked on the host."""
    d, sigma, m, w = problem(p, n, rot)
    cls = (np.arange(p) + rot) % 4
    s2 = sigma * sigma
    assert np.all(np.isfinite(m)) and np.all(np.abs(d) >= 0.25)
    assert np.all(np.isfinite(w)) and np.all(w[:, [0, 1, 2, 3, 5]] >= 0.0)
    assert np.array_equal(sigma == 0.0, cls == 0)
    assert np.all((s2[cls == 1] >= 1e-12 * (1 - 1e-9)) &
                  (s2[cls == 1] <= 1e12 * (1 + 1e-9)))
    assert np.all((s2[cls == 2] >= 1.0) & (s2[cls == 2] < 1.001))
    assert np.all((m == d)[::3, cls == 3])
    rcl = np.arange(n) % 5
    pp = w[:, 3]
    assert np.all(pp[rcl == 0] == 0.0) and np.all(pp[rcl == 1] == 1.0)
    assert np.all(pp[rcl == 2] == 1e-12) and np.all(pp[rcl == 3] == P_TOP)
    assert P_TOP < 1.0 and 1.0 - P_TOP == 2.0**-53
    assert np.all((pp[rcl == 4] >= 1e-3) & (pp[rcl == 4] <= 0.5))
    kinds = expected(p, n, rot)[4]
    assert 0.0 < kinds['v_min'] and kinds['v_max'] < np.inf
    assert 0.0 < kinds['u_min'] and kinds['u_max'] < np.inf
    if p >= 15:
        assert np.all(np.isin(np.arange(4), cls))
        assert np.all(np.isin(np.arange(5), rcl))
        spread = s2[cls == 1]
        assert spread.max() / spread.min() > 1e4
        for kind in ('inlier_far', 'both_far', 'equal', 'p0_outlier_larger',
                     'p1_inlier_larger'):
            assert kinds[kind] >= 1, (kind, kinds)


# ---------------------------------------------------------------- the twin

def _benign(p=40, n=20, seed=0):
    rng = np.random.default_rng(seed)
    d = rng.normal(size=p)
    sigma = 0.5 + rng.random(p)
    m = d + rng.normal(size=(n, p))
    w = np.stack([0.5 + rng.random(n), rng.random(n), 0.1 * rng.random(n),
                  0.05 + 0.4 * rng.random(n), rng.normal(size=n),
                  4.0 + 20.0 * rng.random(n)], axis=1)
    v = w[:, 0:1] * sigma**2 + w[:, 1:2] + w[:, 2:3] * m**2
    u = sigma**2 + w[:, 5:6]
    return d, sigma, m, w, v, u


def test_twin_is_the_logsumexp_of_two_normal_log_densities():
    from scipy.special import logsumexp
    from scipy.stats import norm
    d, sigma, m, w, v, u = _benign()
    p, b = w[:, 3:4], w[:, 4:5]
    like = make(d, sigma, normalised=True)
    t1 = np.log1p(-p) + norm.logpdf(d, m, np.sqrt(v))
    t2 = np.log(p) + norm.logpdf(d, b, np.sqrt(u))
    want = logsumexp(np.stack([t1, t2]), axis=0).sum(axis=1)
    got = like.numpy_from_model(m, w)
    assert np.all(np.abs(got - want) <= 1e-12 * np.abs(want))
    l1, l2 = like.numpy_terms(m, w)
    assert l1.shape == l2.shape == m.shape
    half = 0.5 * np.log(2 * np.pi)
    assert np.allclose(l1 - half, t1, rtol=1e-13, atol=1e-14)
    assert np.allclose(l2 - half, t2, rtol=1e-13, atol=1e-14)
    # numpy() runs the model on the host
    both = GaussianOutlierLikelihood(
        lambda x: (x, torch.from_numpy(w)), d, sigma)
    assert np.array_equal(both.numpy(m), got)


def test_normalisation_is_exactly_the_constant():
    d, sigma, m, w, _, _ = _benign(seed=2)
    raw = make(d, sigma)
    like = make(d, sigma, normalised=True)
    assert raw.log_norm == 0.0
    assert like.log_norm == -0.5 * len(d) * np.log(2 * np.pi)
    assert np.array_equal(like.numpy_from_model(m, w),
                          like.log_norm + raw.numpy_from_model(m, w))


def test_no_outliers_is_the_noise_likelihood():
    """p = 0 against ``GaussianNoiseLikelihood.numpy_from_model`` on the same
    (c, a, f), within the sum of the two budgets, on the p = 0 rows of a GPU
    case: they hold elements whose outlier exponent is the larger one."""
    p, n = 65, 1000
    d, sigma, m, w = problem(p, n)
    rows = np.flatnonzero(w[:, 3] == 0.0)
    assert len(rows) == 200
    m, w = m[rows], w[rows]
    got = make(d, sigma).numpy_from_model(m, w)
    want = GaussianNoiseLikelihood(
        identity, d, sigma, normalised=False).numpy_from_model(m, w[:, :3])
    _, x, a, y, kinds = reference(d, sigma, m, w)
    assert kinds['p0_outlier_larger'] > 0 and np.all(y == 0.0)
    _, nx, na, _, _ = noise_reference(d, sigma, m, w[:, :3], 'row')
    tol = budget(p, x, a, y) + noise_budget(p, nx, na)
    assert np.all(np.isfinite(want))
    used = np.abs(got - want) / tol
    print('largest used fraction of the two budgets %.3g' % used.max())
    assert np.all(used <= 1.0), used.max()


def test_only_outliers_is_the_plain_gaussian_of_the_outlier_component():
    """p = 1: sum_j log N(d_j | b, sigma_j^2 + s) whatever the model says."""
    from scipy.stats import norm
    d, sigma, m, w, _, u = _benign(seed=5)
    w = w.copy()
    w[:, 3] = 1.0
    m = m.copy()
    m[3] = d + 1e6                       # the inlier exponent is -1e11 or so
    m[4, 7] = d[7]                       # ... and here the larger one
    got = make(d, sigma, normalised=True).numpy_from_model(m, w)
    want = norm.logpdf(d, w[:, 4:5], np.sqrt(u)).sum(axis=1)
    assert np.all(np.abs(got - want) <= 1e-12 * np.abs(want))
    l1, _ = make(d, sigma).numpy_terms(m, w)
    assert np.all(l1 == -np.inf)


def test_far_measurements_cost_the_outlier_component_not_minus_infinity():
    d = np.zeros(4)
    sigma = np.ones(4)
    like = make(d, sigma)
    m = np.array([[0.0, 0.0, 0.0, 100.0]])           # 100 sigma
    w = np.array([[1.0, 0.0, 0.0, 0.01, 0.0, 99.0]])
    got = like.numpy_from_model(m, w)[0]
    with np.errstate(divide='ignore'):
        naive = np.log(0.99 * np.exp(-0.5 * m[0]**2) +
                       0.01 * 0.1 * np.exp(-0.5 * d**2 / 100.0))
    assert np.exp(-0.5 * 100.0**2) == 0.0
    assert np.isfinite(got) and abs(got - naive.sum()) < 1e-12
    assert abs(got - (3 * np.log(0.991) + np.log(0.001))) < 1e-12
    # without the outlier component the same row costs 5000
    w[0, 3] = 0.0
    assert like.numpy_from_model(m, w)[0] == -5000.0
    resp = like.numpy_responsibilities(m, np.array([[1, 0, 0, 0.01, 0, 99.0]]))
    assert resp[0, 3] == 1.0 and np.all(resp[0, :3] < 0.0011)


def test_responsibilities():
    d, sigma, m, w, _, _ = _benign(seed=6)
    like = make(d, sigma)
    resp = like.numpy_responsibilities(m, w)
    assert resp.shape == m.shape
    assert np.all((resp > 0) & (resp < 1))
    l1, l2 = like.numpy_terms(m, w)
    assert np.allclose(resp, np.exp(l2) / (np.exp(l1) + np.exp(l2)),
                       rtol=1e-13, atol=0)
    inl = np.exp(l1 - np.logaddexp(l1, l2))
    assert np.all(np.abs(resp + inl - 1.0) <= 4 * EPS)
    # the weights alone decide at p = 0 and p = 1
    w0, w1 = w.copy(), w.copy()
    w0[:, 3], w1[:, 3] = 0.0, 1.0
    assert np.all(like.numpy_responsibilities(m, w0) == 0.0)
    assert np.all(like.numpy_responsibilities(m, w1) == 1.0)
    # a measurement far from the model is an outlier, and the responsibility
    # grows with the residual (f = 0: v does not grow with m)
    wf = w.copy()
    wf[:, 2] = 0.0
    far = m.copy()
    far[:, 0] = d[0] + 30.0
    assert np.all(like.numpy_responsibilities(far, wf)[:, 0] > 1 - 1e-12)
    step = m[:1].repeat(5, axis=0)
    step[:, 1] = d[1] + np.arange(5.0)
    assert np.all(np.diff(like.numpy_responsibilities(
        step, wf[:1].repeat(5, axis=0))[:, 1]) > 0)


def test_twin_nan_rules():
    d, sigma, m, w, _, _ = _benign(seed=3)
    sigma = sigma.copy()
    sigma[5] = 0.0
    like = make(d, sigma)
    clean = like.numpy_from_model(m, w)
    assert np.all(np.isfinite(clean))
    m, w = m.copy(), w.copy()
    m[1, 0] = np.nan
    m[2, 7] = np.inf
    m[3, 39] = -np.inf
    w[4, :3] = [1.0, 0.0, 0.0]             # v = 0 in column 5
    w[5, 5] = 0.0                          # u = 0 in column 5
    w[6, :3] = [1.0, -10.0, 0.0]           # negative v
    w[7, 1] = np.inf
    w[8, 0] = np.nan
    w[9, :3] = [-1.0, 5.0, 0.0]            # a negative coefficient, v > 0
    w[10, 3] = -1e-300                     # p below 0
    w[11, 3] = 1.0 + 2.0**-52              # p above 1
    w[12, 3] = np.nan
    w[13, 4] = np.inf                      # b
    w[14, 4] = np.nan
    w[15, 5] = -10.0                       # negative u
    w[16, 5] = np.inf
    w[17, 5] = np.nan
    w[18, 5] = -0.2                        # a negative s, u > 0 but in col. 5
    w[19, 3:] = [0.0, np.nan, 1.0]         # b counts also where p = 0
    bad = [1, 2, 3, 4, 5, 6, 7, 8] + list(range(10, 20))
    out = like.numpy_from_model(m, w)
    assert np.array_equal(np.flatnonzero(np.isnan(out)), bad)
    assert out[0] == clean[0] and np.isfinite(out[9])
    l1, l2 = like.numpy_terms(m, w)
    assert np.array_equal(np.isnan(l1), np.isnan(l2))
    assert np.array_equal(np.isnan(l1).any(axis=1), np.isnan(out))
    assert np.array_equal(np.isnan(like.numpy_responsibilities(m, w)),
                          np.isnan(l1))
    # a row of the rules above is NaN in all its elements where a row
    # coefficient is to blame, in one where an element is
    assert np.all(np.isnan(l1[12])) and np.sum(np.isnan(l1[1])) == 1
    # p = 0 and p = 1 are legal whatever the other exponent is
    m[0] = d + 1e8
    w[0, 3] = 1.0
    assert np.isfinite(like.numpy_from_model(m, w)[0])
    m[0] = d
    w[0, 3:] = [0.0, 1e200, 1.0]
    assert np.isfinite(like.numpy_from_model(m, w)[0])


def test_constructor_errors():
    d = np.array([0.5, -1.0, 2.0])
    s = np.array([0.1, 0.0, 0.3])
    assert make(d, s).n_data == 3
    assert np.all(make(d, None).sigma == 0.0)
    with pytest.raises(ValueError):
        GaussianOutlierLikelihood(None, d, s)
    with pytest.raises(TypeError):
        GaussianOutlierLikelihood(identity, d, s, False)
    for bad in (np.zeros(0), np.zeros((3, 1)), np.r_[0.5, np.nan, 1.0],
                np.r_[0.5, np.inf, 1.0], np.zeros((1 << 20) + 1)):
        with pytest.raises(ValueError):
            GaussianOutlierLikelihood(identity, bad, None)
    assert GaussianOutlierLikelihood(identity, np.zeros(1 << 20)).n_data == \
        1 << 20
    for bad in (np.r_[0.1, -0.1, 0.3], np.r_[0.1, np.nan, 0.3],
                np.r_[0.1, np.inf, 0.3], np.r_[0.1, 1e200, 0.3], np.ones(4),
                np.ones((3, 1))):
        with pytest.raises(ValueError):
            GaussianOutlierLikelihood(identity, d, bad)
    like = make(d, s)
    m = np.zeros((4, 3))
    for args in ((m[:, :2], np.ones((4, 6))), (m, np.ones((4, 5))),
                 (m, np.ones((4, 7))), (m, np.ones((3, 6))),
                 (m[0], np.ones((4, 6))), (m, np.ones(6))):
        for fn in (like.numpy_from_model, like.numpy_terms,
                   like.numpy_responsibilities):
            with pytest.raises(ValueError):
                fn(*args)


def test_pickle_drops_the_device_tables():
    d, sigma, m, w, _, _ = _benign(seed=4)
    like = make(d, sigma, normalised=True)
    like._tables[0] = object()
    again = pickle.loads(pickle.dumps(like))
    assert again._tables == {} and like._tables
    assert again.log_norm == like.log_norm
    assert np.array_equal(again.numpy_from_model(m, w),
                          like.numpy_from_model(m, w))


def test_exported_lazily():
    import nautilus_amd
    assert 'GaussianOutlierLikelihood' in nautilus_amd.__all__
    assert nautilus_amd.GaussianOutlierLikelihood is GaussianOutlierLikelihood
    assert GaussianOutlierLikelihood.device is True
    assert GaussianOutlierLikelihood._pair is True


def test_header_and_binding_declare_the_entry():
    import os
    from nautilus_amd import _lib, device
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, 'include', 'nautilus_hip.h')).read()
    assert '#define NB_OUTLIER_WIDTH 6' in header
    assert 'int nb_outlier_loglike(const nb_noise* h,' in header
    assert 'nb_outlier_loglike' in _lib.exported_symbols()
    assert device.OUTLIER_WIDTH == 6


# ------------------------------------------- the budget and the GPU inputs

def _twin_in_budget(p, d, sigma, m, w, ref):
    want, x, a, y, _ = ref
    got = make(d, sigma).numpy_from_model(m, w)
    tol = budget(p, x, a, y)
    assert np.all(np.isfinite(want)) and np.all(tol > 0)
    assert np.all(np.isfinite(got))
    used = np.abs(got - want) / tol
    print('P = %d, n = %d: the twin uses %.3g of the bound' % (
        p, len(m), used.max()))
    assert np.all(used <= 1.0), used.max()


@pytest.mark.parametrize('p, n, rot', SHAPES)
def test_twin_stays_inside_the_budget(p, n, rot):
    check_classes(p, n, rot)
    _twin_in_budget(p, *problem(p, n, rot), expected(p, n, rot))


def test_twin_stays_inside_the_budget_on_the_long_row():
    d, sigma, m, w = long_problem(*LONG_SHAPE)
    ref = long_expected()
    assert 1.0 <= ref[4]['b_min'] and ref[4]['b_max'] < 1.001
    _twin_in_budget(LONG_SHAPE[0], d, sigma, m, w, ref)


@pytest.mark.parametrize('p, n', [(p, 4097) for p in ROW_TEST_P] +
                         [(p, 1000) for p in EDGE_TEST_P])
def test_twin_stays_inside_the_budget_on_the_other_gpu_inputs(p, n):
    check_classes(p, n, 0)
    _twin_in_budget(p, *problem(p, n), expected(p, n))


def test_the_naive_form_fails_where_the_twin_does_not():
    """log(w1 N1 + w2 N2) is -inf in the rows that hold an element with both
    exponents below -745: the budget is not met by any formula."""
    p, n = 65, 1000
    d, sigma, m, w = problem(p, n)
    want, _, _, _, kinds = expected(p, n)
    assert kinds['both_far'] > 0
    like = make(d, sigma)
    l1, l2 = like.numpy_terms(m, w)
    with np.errstate(divide='ignore'):
        naive = np.log(np.exp(l1) + np.exp(l2)).sum(axis=1)
    assert np.sum(np.isinf(naive)) >= n // 7
    assert np.all(np.isfinite(like.numpy_from_model(m, w)))
