"""Host side of ``GaussianNoiseLikelihood``: the numpy twin against scipy, the
data-vector likelihood and ``np.longdouble``, its NaN rules, constructor
validation and pickling; and the problems, the reference and the error budget
that test_noise_likelihood_gpu.py holds the device kernel to."""

import functools
import math
import pickle

import numpy as np
import pytest
import torch

from nautilus_amd import GaussianDataLikelihood, GaussianNoiseLikelihood

EPS = 2.0**-52
TINY = 2.0**-100

# every P and every n of the two lists appears; the kernel changes its shape
# (L, R, U) after P = 32 and after P = 512 (device.noise_launch_shape)
P_ALL = (1, 3, 15, 16, 17, 32, 33, 63, 64, 65, 257, 512, 513, 1025, 4099)
N_ALL = (1, 15, 17, 1000, 4097)
# (P, n, rot): a column's class is (j + rot) % 4, see problem().  From P = 15
# on a case holds every class; P = 1 and P = 3 cannot, and run once per rot
# instead.  The order of the long P keeps n P below 4.3 million.
_P_LONG = (15, 16, 17, 32, 33, 63, 64, 65, 4099, 257, 512, 513, 1025)
SHAPES = [(p, N_ALL[(i + s) % 5], 0) for i, p in enumerate(_P_LONG)
          for s in (0, 2)] + \
    [(p, N_ALL[(rot + p) % 5], rot) for p in (1, 3) for rot in range(4)]
assert {s[0] for s in SHAPES} == set(P_ALL)
assert {s[1] for s in SHAPES} == set(N_ALL)
assert max(s[0] * s[1] for s in SHAPES) < 4.3e6
MODES = ('row', 'full')
# rows that a lane's running product cannot hold without renormalising: every
# v in [1, 1.001) has a mantissa near 1/2.  At P = 131075 a lane of a
# wavefront-wide row sees 2049 elements, 513 per product; at P = 1048573 a
# product sees 4096, which 2^-4096 would underflow.
LONG_SHAPES = [(131075, 33), (1048573, 5)]
# what the bit-for-bit and the edge tests of the GPU file read
ROW_TEST_P = (3, 129, 1025)
EDGE_TEST_P = (17, 129, 1025)


def identity(x):
    return x


@functools.lru_cache(maxsize=4)
def problem(p, n, mode, rot=0):
    """Data, sigma, n model rows and their noise.  Column j is of class
    (j + rot) % 4:
      0  sigma_j = 0;
      1  sigma_j^2 log-uniform in [1e-12, 1e12];
      2  sigma_j^2 in [1, 1.001);
      3  sigma_j^2 log-uniform in [0.01, 100], and m = d exactly in every
         third row.
    Row i is of class i % 4, with c in [1/2, 2), a log-uniform in [1e-3, 10]
    and f log-uniform in [1e-4, 0.1] unless the class says otherwise:
      0  c = 0;   1  a = 0;   2  f = 0;   3  (c, a, f) = (1, 2^-100, 0).
    In full mode w_ij = a_i (1 + u_ij) + f_i m_ij^2 with the same a and f (and
    c = 1).  Every coefficient is >= 0, so no v cancels, and |d| >= 1/4, so
    that f m^2 alone keeps v > 0.  The residuals are of the size of the error
    bars: m = d + sqrt(v(d)) N(0, 1).  Nobody writes to the result."""
    rng = np.random.default_rng(1000003 * rot + 1000 * p + n +
                                (500 if mode == 'full' else 0))
    cls = (np.arange(p) + rot) % 4
    s2 = 10.0**rng.uniform(-2, 2, size=p)
    s2[cls == 0] = 0.0
    k = int(np.sum(cls == 1))                   # one per stratum of the range
    s2[cls == 1] = 10.0**(rng.permutation(
        (np.arange(k) + rng.random(k)) / max(k, 1)) * 24 - 12)
    s2[cls == 2] = (1.00001 + 0.00098 * rng.random(p))[cls == 2]
    sigma = np.sqrt(s2)
    d = (0.25 + rng.exponential(size=p)) * rng.choice([-1.0, 1.0], size=p)
    rcl = np.arange(n) % 4
    c = 0.5 + 1.5 * rng.random(n)
    a = 10.0**rng.uniform(-3, 1, size=n)
    f = 10.0**rng.uniform(-4, -1, size=n)
    c[rcl == 0] = 0.0
    a[rcl == 1] = 0.0
    f[rcl == 2] = 0.0
    c[rcl == 3], a[rcl == 3], f[rcl == 3] = 1.0, TINY, 0.0
    if mode == 'full':
        c[:] = 1.0
    scale = np.sqrt(c[:, None] * s2 + a[:, None] + f[:, None] * d * d)
    m = d + scale * rng.normal(size=(n, p))
    exact = (np.arange(n) % 3 == 0)[:, None] & (cls == 3)
    m = np.where(exact, d, m)
    if mode == 'full':
        w = a[:, None] * (1.0 + rng.random((n, p))) + f[:, None] * m * m
        w[rcl == 3] = TINY
    else:
        w = np.stack([c, a, f], axis=1)
    for arr in (d, sigma, m, w):
        arr.setflags(write=False)
    return d, sigma, m, w


def long_problem(p, n):
    """Row mode with every v in [1, 1.001): sigma^2 in [1, 1.0005), c = 1, a
    below 5e-4, f = 0."""
    rng = np.random.default_rng(p + n)
    sigma = np.sqrt(1.00001 + 0.00048 * rng.random(p))
    d = rng.normal(size=p)
    w = np.stack([np.ones(n), 5e-4 * rng.random(n), np.zeros(n)], axis=1)
    m = d + rng.normal(size=(n, p))
    return d, sigma, m, w


def zero_residual_problem(p, mode):
    """Row 6 of ``problem(p, 1000, mode)`` with m = d in every column (in
    full mode with w = 1/4, so that v > 0 where sigma_j = 0): one row."""
    d, sigma, m, w = problem(p, 1000, mode)
    w = w[6:7].copy()
    if mode == 'full':
        w[0] = 0.25
    return d, sigma, d[None].copy(), w


def unit_inflation_problem():
    """The columns of ``problem(257, 1000, 'row')`` with sigma_j > 0, and
    (c, a, f) = (1, 0, 0) in every row: what ``GaussianDataLikelihood`` can
    express too."""
    d, sigma, m, _ = problem(257, 1000, 'row')
    pos = sigma > 0
    w = np.tile([1.0, 0.0, 0.0], (len(m), 1))
    return d[pos], sigma[pos], np.ascontiguousarray(m[:, pos]), w


def reference(d, sigma, m, w, mode):
    """The defining formula in ``np.longdouble`` from the float64 inputs:
    log L without the constant, rounded once, and per row X = sum_j r^2 / v,
    A = sum_j |log v| and the extremes of v."""
    ld = np.longdouble
    s2 = sigma.astype(ld)**2
    ml = m.astype(ld)
    wl = w.astype(ld)
    if mode == 'row':
        v = wl[:, 0:1] * s2 + wl[:, 1:2] + wl[:, 2:3] * ml * ml
    else:
        v = s2 + wl
    r = ml - d.astype(ld)
    chi = r * r / v
    log_v = np.log(v)
    out = (-0.5 * (chi + log_v).sum(axis=1)).astype(float)
    return out, chi.sum(axis=1).astype(float), \
        np.abs(log_v).sum(axis=1).astype(float), \
        float(v.min()), float(v.max())


@functools.lru_cache(maxsize=None)
def expected(p, n, mode, rot=0):
    """``reference`` of ``problem(p, n, mode, rot)``: rows only, computed once
    and shared by both test files."""
    return reference(*problem(p, n, mode, rot), mode)


@functools.lru_cache(maxsize=None)
def long_expected(p, n):
    return reference(*long_problem(p, n), 'row')


def budget(p, x, a):
    """The bound on |log L_device - log L_true| of a row, a function of the
    inputs only:

        tol = eps (4 X + A + 4 P) + 1/2 eps (T + 2) (X + A),

    X = sum_j r^2 / v, A = sum_j |log v|, eps = 2^-52 (every rounding errs by
    at most eps / 2 of its result), log L = -1/2 S with S = sum_j (r^2 / v +
    log v), so an error of S counts half.

    Per element.  v: sigma^2 is rounded on the host (1/2 eps of c sigma^2),
    m^2 (1/2), the inner fma (1/2 of c sigma^2 + a) and the outer one (1/2 of
    v); all terms are >= 0, so v errs by at most 3/2 eps v.  r = m - d (1/2,
    so r^2 carries 1), r r (1/2), 1 / v after two Newton steps (3/4) and the
    last product (1/2): with v's 3/2 the term r^2 / v errs by 17/4 eps of
    itself, 17/8 eps X in log L <= 4 eps X.  log v inherits 3/2 eps from v,
    absolutely; v's mantissa enters a product by one multiplication (1/2 eps
    relative to the product, 1/2 eps in its log): 2 eps P in S.  Moving the
    product's exponent to the integer sum is exact.
    Per product (L U of them per row).  One po_log of a number in (2^-257, 1],
    within 1 ulp: eps |lg| with |lg| <= log 2 times the elements multiplied
    since the last renormalisation, <= 0.7 eps P over the row.  The integer
    exponent E times the double nearest log 2, joined by one fma: 1/2 eps E
    log 2 for the constant and 1/2 eps of the result, a partial sum of the log
    v; with |E log 2| <= |partial sum| + |lg| that is eps A + 0.35 eps P.
    Together 3.05 eps P + eps A in S, half of it in log L: <= eps (4 P + A).
    Sums.  A row's chi^2 partial takes one addition per step, ceil(P / (L U))
    of them, then one to join the log, log2(U) in the tree, log2(L) across
    the lanes and one for the constant: T + 2 additions, T = ceil(P / (L U))
    + log2(L U), each erring by eps / 2 of a partial sum that is at most
    X + A in size (1/4 eps (T + 2) (X + A) in log L, the budget grants
    twice that).  T is capped at P / 16 + 8."""
    from nautilus_amd import device
    lanes, _, u = device.noise_launch_shape(p)
    t = min(math.ceil(p / (lanes * u)) + math.log2(lanes * u), p / 16 + 8)
    return EPS * (4 * x + a + 4 * p) + 0.5 * EPS * (t + 2) * (x + a)


def make(d, sigma, mode, normalised=False):
    return GaussianNoiseLikelihood(identity, d, sigma, noise=mode,
                                   normalised=normalised)


def check_classes(p, n, mode, rot):
    """What a case of ``problem`` holds, checked on the host."""
    d, sigma, m, w = problem(p, n, mode, rot)
    cls = (np.arange(p) + rot) % 4
    s2 = sigma * sigma
    assert np.all(np.isfinite(m)) and np.all(np.abs(d) >= 0.25)
    assert np.all(w >= 0.0) and np.all(np.isfinite(w))
    assert np.array_equal(sigma == 0.0, cls == 0)
    assert np.all((s2[cls == 1] >= 1e-12 * (1 - 1e-9)) &
                  (s2[cls == 1] <= 1e12 * (1 + 1e-9)))
    assert np.all((s2[cls == 2] >= 1.0) & (s2[cls == 2] < 1.001))
    assert np.all((m == d)[::3, cls == 3])
    if p >= 15:
        assert np.all(np.isin(np.arange(4), cls))
        spread = s2[cls == 1]
        assert spread.max() / spread.min() > 1e4
    rcl = np.arange(n) % 4
    if mode == 'row':
        assert np.array_equal(w[:, 0] == 0.0, rcl == 0)
        assert np.array_equal(w[:, 1] == 0.0, rcl == 1)
        assert np.array_equal(w[:, 2] == 0.0, (rcl == 2) | (rcl == 3))
        assert np.all(w[rcl == 3] == np.array([1.0, TINY, 0.0]))
    else:
        assert np.all(w[rcl == 3] == TINY)
    _, _, _, v_min, v_max = expected(p, n, mode, rot)
    assert 0.0 < v_min and v_max < np.inf


# ---------------------------------------------------------------- the twin

def _benign(mode, p=40, n=20, seed=0):
    rng = np.random.default_rng(seed)
    d = rng.normal(size=p)
    sigma = 0.5 + rng.random(p)
    m = d + rng.normal(size=(n, p))
    if mode == 'row':
        w = np.stack([0.5 + rng.random(n), rng.random(n),
                      0.1 * rng.random(n)], axis=1)
        v = w[:, 0:1] * sigma**2 + w[:, 1:2] + w[:, 2:3] * m**2
    else:
        w = rng.random((n, p))
        v = sigma**2 + w
    return d, sigma, m, w, v


@pytest.mark.parametrize('mode', MODES)
def test_twin_is_the_sum_of_normal_log_densities(mode):
    from scipy.stats import norm
    d, sigma, m, w, v = _benign(mode)
    like = make(d, sigma, mode, normalised=True)
    want = norm.logpdf(d, m, np.sqrt(v)).sum(axis=1)
    got = like.numpy_from_model(m, w)
    assert np.all(np.abs(got - want) <= 1e-12 * np.abs(want))
    chi, log_v = like.numpy_terms(m, w)
    assert chi.shape == log_v.shape == m.shape
    assert np.allclose(chi, (m - d)**2 / v, rtol=1e-14, atol=0)
    assert np.allclose(log_v, np.log(v), rtol=1e-14, atol=1e-16)
    # numpy() runs the model on the host
    both = GaussianNoiseLikelihood(
        lambda x: (x, torch.from_numpy(w)), d, sigma, noise=mode)
    assert np.array_equal(both.numpy(m), got)


def test_unit_inflation_is_the_data_vector_likelihood():
    d, sigma, m, _, _ = _benign('row', seed=1)
    w = np.tile([1.0, 0.0, 0.0], (len(m), 1))
    want = GaussianDataLikelihood(identity, d, sigma=sigma).numpy_from_model(m)
    got = make(d, sigma, 'row', normalised=True).numpy_from_model(m, w)
    assert np.all(np.abs(got - want) <= 1e-12 * np.abs(want))
    full = make(d, sigma, 'full', normalised=True).numpy_from_model(
        m, np.zeros_like(m))
    assert np.all(np.abs(full - want) <= 1e-12 * np.abs(want))


def test_normalisation_is_exactly_the_constant():
    d, sigma, m, w, _ = _benign('row', seed=2)
    raw = make(d, sigma, 'row')
    like = make(d, sigma, 'row', normalised=True)
    assert raw.log_norm == 0.0
    assert like.log_norm == -0.5 * len(d) * np.log(2 * np.pi)
    assert np.array_equal(like.numpy_from_model(m, w),
                          like.log_norm + raw.numpy_from_model(m, w))


@pytest.mark.parametrize('mode', MODES)
def test_twin_nan_rules(mode):
    d, sigma, m, w, _ = _benign(mode, seed=3)
    sigma = sigma.copy()
    sigma[5] = 0.0
    like = make(d, sigma, mode)
    clean = like.numpy_from_model(m, w)
    assert np.all(np.isfinite(clean))
    m, w = m.copy(), w.copy()
    m[1, 0] = np.nan
    m[2, 7] = np.inf
    m[3, 39] = -np.inf
    if mode == 'row':
        w[4] = [1.0, 0.0, 0.0]             # v = 0 in column 5
        w[6] = [1.0, -10.0, 0.0]           # negative v
        w[7, 1] = np.inf
        w[8, 0] = np.nan
        w[9] = [-1.0, 5.0, 0.0]            # a negative coefficient, v > 0
        bad = [1, 2, 3, 4, 6, 7, 8]
    else:
        w[4, 5] = 0.0                      # v = 0: sigma_5 = 0
        w[6, 3] = -10.0
        w[7, 11] = np.inf
        w[8, 12] = np.nan
        w[9, 3] = -0.01                    # a negative w, v > 0
        bad = [1, 2, 3, 4, 6, 7, 8]
    out = like.numpy_from_model(m, w)
    assert np.array_equal(np.flatnonzero(np.isnan(out)), bad)
    keep = np.ones(len(m), bool)
    keep[bad + [9]] = False
    assert np.array_equal(out[keep], clean[keep])
    assert np.isfinite(out[9])
    chi, log_v = like.numpy_terms(m, w)
    assert np.array_equal(np.isnan(chi), np.isnan(log_v))
    assert np.array_equal(np.isnan(chi).any(axis=1), np.isnan(out))
    # r = 0 with v > 0 adds only the log v
    m[0] = d
    chi, log_v = like.numpy_terms(m, w)
    assert np.all(chi[0] == 0.0) and np.all(np.isfinite(log_v[0]))


def test_constructor_errors():
    d = np.array([0.5, -1.0, 2.0])
    s = np.array([0.1, 0.0, 0.3])
    assert make(d, s, 'row').n_data == 3
    assert np.all(make(d, None, 'full').sigma == 0.0)
    with pytest.raises(ValueError):
        GaussianNoiseLikelihood(None, d, s)
    with pytest.raises(ValueError):
        GaussianNoiseLikelihood(identity, d, s, noise='column')
    for bad in (np.zeros(0), np.zeros((3, 1)), np.r_[0.5, np.nan, 1.0],
                np.r_[0.5, np.inf, 1.0], np.zeros((1 << 20) + 1)):
        with pytest.raises(ValueError):
            GaussianNoiseLikelihood(identity, bad, None)
    assert GaussianNoiseLikelihood(identity, np.zeros(1 << 20)).n_data == \
        1 << 20
    for bad in (np.r_[0.1, -0.1, 0.3], np.r_[0.1, np.nan, 0.3],
                np.r_[0.1, np.inf, 0.3], np.r_[0.1, 1e200, 0.3], np.ones(4),
                np.ones((3, 1))):
        with pytest.raises(ValueError):
            GaussianNoiseLikelihood(identity, d, bad)
    like = make(d, s, 'row')
    m = np.zeros((4, 3))
    for args in ((m[:, :2], np.ones((4, 3))), (m, np.ones((4, 2))),
                 (m, np.ones((3, 3))), (m[0], np.ones((4, 3))),
                 (m, np.ones(3))):
        with pytest.raises(ValueError):
            like.numpy_from_model(*args)
    with pytest.raises(ValueError):
        make(d, s, 'full').numpy_from_model(m, np.ones((4, 2)))


def test_pickle_drops_the_device_tables():
    d, sigma, m, w, _ = _benign('row', seed=4)
    like = make(d, sigma, 'row', normalised=True)
    like._tables[0] = object()
    again = pickle.loads(pickle.dumps(like))
    assert again._tables == {} and like._tables
    assert again.noise == 'row' and again.log_norm == like.log_norm
    assert np.array_equal(again.numpy_from_model(m, w),
                          like.numpy_from_model(m, w))


def test_exported_lazily():
    import nautilus_amd
    assert 'GaussianNoiseLikelihood' in nautilus_amd.__all__
    assert nautilus_amd.GaussianNoiseLikelihood is GaussianNoiseLikelihood
    assert GaussianNoiseLikelihood.device is True


# ------------------------------------------- the budget and the GPU inputs

def _twin_in_budget(p, d, sigma, m, w, mode, ref):
    want, x, a = ref[:3]
    got = make(d, sigma, mode).numpy_from_model(m, w)
    tol = budget(p, x, a)
    assert np.all(np.isfinite(want)) and np.all(tol > 0)
    used = np.abs(got - want) / tol
    print('P = %d, n = %d, %s: the twin uses %.3g of the bound' % (
        p, len(m), mode, used.max()))
    assert np.all(used <= 1.0), used.max()


@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('p, n, rot', SHAPES)
def test_twin_stays_inside_the_budget(p, n, rot, mode):
    check_classes(p, n, mode, rot)
    _twin_in_budget(p, *problem(p, n, mode, rot), mode,
                    expected(p, n, mode, rot))


@pytest.mark.parametrize('p, n', LONG_SHAPES)
def test_twin_stays_inside_the_budget_on_long_rows(p, n):
    d, sigma, m, w = long_problem(p, n)
    ref = long_expected(p, n)
    assert 1.0 <= ref[3] and ref[4] < 1.001
    _twin_in_budget(p, d, sigma, m, w, 'row', ref)


@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('p, n', [(p, 4097) for p in ROW_TEST_P] +
                         [(p, 1000) for p in EDGE_TEST_P] + [(257, 1000)])
def test_twin_stays_inside_the_budget_on_the_other_gpu_inputs(p, n, mode):
    check_classes(p, n, mode, 0)
    _twin_in_budget(p, *problem(p, n, mode), mode, expected(p, n, mode))


@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('p', EDGE_TEST_P)
def test_twin_stays_inside_the_budget_at_zero_residuals(p, mode):
    d, sigma, m, w = zero_residual_problem(p, mode)
    ref = reference(d, sigma, m, w, mode)
    assert ref[1][0] == 0.0 and ref[3] > 0
    _twin_in_budget(p, d, sigma, m, w, mode, ref)


def test_twin_stays_inside_the_budget_at_unit_inflation():
    d, sigma, m, w = unit_inflation_problem()
    assert np.all(sigma > 0) and 150 < len(d) < 257
    _twin_in_budget(len(d), d, sigma, m, w, 'row',
                    reference(d, sigma, m, w, 'row'))
