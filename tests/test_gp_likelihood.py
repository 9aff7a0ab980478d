"""Host side of ``GaussianProcessLikelihood``: the numpy twin against the
defining formula in ``np.longdouble``, scipy and the data-vector likelihood,
its NaN rules, constructor validation and pickling; and the problems, the
reference and the error budget that test_gp_likelihood_gpu.py holds the device
kernel to."""

import functools
import pickle
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from nautilus_amd import GaussianDataLikelihood, GaussianProcessLikelihood
from nautilus_amd.likelihoods import GP_KERNELS, N_GP_MAX, gp_correlation

EPS = 2.0**-52
MODES = ('hyper', 'full')
# both sides of every multiple of 16: the kernel is instantiated per tile
# count ceil(P / 16) (device.gp_launch_shape)
P_ALL = (1, 2, 15, 16, 17, 32, 33, 48, 49, 64, 65, 80, 81, 96, 97, 112, 113,
         127, 128)
N_ALL = (1, 3, 17, 130)
# (P, n, kernel, rot): every P twice, with kernels two apart, so that the two
# or more P of a tile count meet all four kernels; a column's class is
# (j + rot) % 3, see problem()
SHAPES = [(p, N_ALL[(i + s) % 4], GP_KERNELS[(i + s) % 4], s // 2)
          for i, p in enumerate(P_ALL) for s in (0, 2)]
assert {s[0] for s in SHAPES} == set(P_ALL)
assert {s[1] for s in SHAPES} == set(N_ALL)
assert {((s[0] + 15) // 16, s[2]) for s in SHAPES} == \
    {(t, k) for t in range(1, 9) for k in GP_KERNELS}
assert max(s[0]**2 * s[1] for s in SHAPES) < 4.3e6
P_2D = 33                                 # the P whose t is two-dimensional
# what the bit-for-bit and the edge tests of the GPU file read
ROW_TEST = {'hyper': ((3, 33, 128), 4097), 'full': ((3, 33), 257)}
EDGE_TEST_P = (17, 65, 128)
# roundings of one off-diagonal element of K in hyper mode, in units of EPS:
# see budget()
C_B = 8


def identity(x):
    return x


def make(t, d, sigma, mode, kernel='sqexp', normalised=False):
    return GaussianProcessLikelihood(identity, t, d, sigma, kernel=kernel,
                                     cov=mode, normalised=normalised)


def locations(p, rng):
    if p == P_2D:
        return rng.uniform(0, 10, size=(p, 2))
    return np.sort(rng.uniform(0, 10, size=p))


def hyper_rows(p, n, dist, rng):
    """(a, l, s) of n rows; row i is of class i % 4:
      0  a = 0 (white noise only), s log-uniform in [1e-3, 1];
      1  l = 0.2 of the median distance to the nearest neighbour: K is nearly
         diagonal;
      2  l about the span of t: K is nearly of rank one, plus noise;
      3  generic.
    Unless the class says otherwise a is log-uniform in [0.1, 10], l in
    [0.2, 3] and s in [1e-6, 0.1] a."""
    a = 10.0**rng.uniform(-1, 1, size=n)
    l = 10.0**rng.uniform(np.log10(0.2), np.log10(3.0), size=n)
    s = a * 10.0**rng.uniform(-6, -1, size=n)
    rcl = np.arange(n) % 4
    if p > 1:
        near = np.median(np.min(dist + np.diag(np.full(p, np.inf)), axis=1))
        span = dist.max()
    else:
        near, span = 1.0, 10.0
    a[rcl == 0] = 0.0
    s[rcl == 0] = 10.0**rng.uniform(-3, 0, size=n)[rcl == 0]
    l[rcl == 1] = 0.2 * near
    l[rcl == 2] = span * (0.8 + 0.4 * rng.random(n))[rcl == 2]
    return np.stack([a, l, s], axis=1)


@functools.lru_cache(maxsize=4)
def problem(p, n, mode, kernel, rot=0):
    """Locations, data, sigma, n model rows and their covariance input,
    deterministic from the arguments.  t is sorted uniform on [0, 10] (at
    P = 33 uniform on [0, 10]^2).  Column j is of class (j + rot) % 3:
      0  sigma_j = 0;
      1  sigma_j^2 log-uniform in [1e-8, 1e4];
      2  sigma_j^2 in [0.01, 0.01001).
    The rows are those of ``hyper_rows``.  In full mode C is the same
    a rho(D / l) + s I built in float64 in the even rows, and in the odd rows
    a random symmetric positive definite Q diag(lambda) Q^T with lambda
    log-uniform in [1e-3, 1e3].  The residuals are drawn as L z with K =
    L L^T and z standard normal, so that r^T K^-1 r is about P.  Nobody writes
    to the result."""
    rng = np.random.default_rng([p, n, MODES.index(mode),
                                 GP_KERNELS.index(kernel), rot])
    t = locations(p, rng)
    cls = (np.arange(p) + rot) % 3
    k1 = int(np.sum(cls == 1))                  # one per stratum of the range
    s2 = np.zeros(p)
    s2[cls == 1] = 10.0**(rng.permutation(
        (np.arange(k1) + rng.random(k1)) / max(k1, 1)) * 12 - 8)
    s2[cls == 2] = (0.01 * (1.0 + 0.001 * rng.random(p)))[cls == 2]
    sigma = np.sqrt(s2)
    d = rng.normal(size=p)
    bare = make(t, d, None, 'hyper', kernel)
    h = hyper_rows(p, n, bare.dist, rng)
    c = bare.numpy_covariance(np.zeros((n, p)), h)      # a rho(D / l) + s I
    for i in range(1, n if mode == 'full' else 0, 2):
        q, _ = np.linalg.qr(rng.normal(size=(p, p)))
        c[i] = (q * 10.0**rng.uniform(-3, 3, size=p)) @ q.T
        c[i] = 0.5 * (c[i] + c[i].T)
    chol = np.linalg.cholesky(c + np.diag(sigma * sigma))
    m = d + np.einsum('nij,nj->ni', chol, rng.normal(size=(n, p)))
    cov = h if mode == 'hyper' else c
    for arr in (t, d, sigma, m, cov):
        arr.setflags(write=False)
    return t, d, sigma, m, cov


def row_problem(p, n, mode, kernel='matern32'):
    """Many rows for the bit-for-bit tests, without their (n, P, P)
    covariances in hyper mode: the rows of ``hyper_rows`` and m = d + N(0, 1)."""
    if mode == 'full':
        return problem(p, n, mode, kernel)
    rng = np.random.default_rng([p, n, 77])
    t = locations(p, rng)
    sigma = np.sqrt(10.0**rng.uniform(-4, 0, size=p))
    d = rng.normal(size=p)
    h = hyper_rows(p, n, make(t, d, None, 'hyper').dist, rng)
    return t, d, sigma, d + rng.normal(size=(n, p)), h


def reference(dist, d, sigma, m, cov, mode, kernel):
    """The defining formula in ``np.longdouble`` from the float64 inputs (the
    distances as the likelihood keeps them): the kernel function in long
    double, an outer-product Cholesky vectorised over the rows, log L without
    the constant rounded once.  Also, for the budget and in float64: q =
    r^T K^-1 r, alpha = K^-1 r, y = L^-1 r, K^-1, |L| and diag K per row (K^-1
    from the rounded factor by LAPACK: a bound needs its leading digits
    only)."""
    from scipy.linalg import solve_triangular
    ld = np.longdouble
    n, p = m.shape
    diag = np.arange(p)
    s2 = sigma.astype(ld)**2
    if mode == 'hyper':
        a, l, s = (cov[:, i].astype(ld)[:, None, None] for i in range(3))
        k = a * gp_correlation(kernel, dist.astype(ld) / l)
        k[:, diag, diag] = a[:, 0] + s2 + s[:, 0]
    else:
        low = np.tril(cov.astype(ld))
        k = low + np.transpose(np.tril(low, -1), (0, 2, 1))
        k[:, diag, diag] += s2
    k_diag = k[:, diag, diag].astype(float)
    r = m.astype(ld) - d.astype(ld)
    low = np.zeros_like(k)
    y = np.zeros_like(r)
    for j in range(p):
        piv = k[:, j, j]
        assert np.all(piv > 0)
        ljj = np.sqrt(piv)
        col = k[:, j:, j] / ljj[:, None]
        low[:, j:, j] = col
        y[:, j] = r[:, j] / ljj
        r[:, j + 1:] -= col[:, 1:] * y[:, j, None]
        k[:, j + 1:, j + 1:] -= col[:, 1:, None] * col[:, None, 1:]
    log_diag = np.log(low[:, diag, diag])
    q = np.sum(y * y, axis=1)
    out = (-0.5 * (q + 2 * log_diag.sum(axis=1))).astype(float)
    lf, yf = low.astype(float), y.astype(float)
    inv = np.stack([solve_triangular(x, np.eye(p), lower=True) for x in lf])
    return SimpleNamespace(
        out=out, q=q.astype(float), y=yf, abs_l=np.abs(lf), k_diag=k_diag,
        alpha=np.einsum('nji,nj->ni', inv, yf),
        k_inv=np.einsum('nji,njk->nik', inv, inv))


@functools.lru_cache(maxsize=None)
def expected(p, n, mode, kernel, rot=0):
    """``reference`` of ``problem(p, n, mode, kernel, rot)``: computed once
    and shared by both test files."""
    t, d, sigma, m, cov = problem(p, n, mode, kernel, rot)
    return reference(make(t, d, None, 'hyper').dist, d, sigma, m, cov, mode,
                     kernel)


def budget(p, ref, a=None):
    """The bound on |log L_computed - log L_true| of every row, a function of
    the inputs only; eps = 2^-52, gamma_k = k eps / (1 - k eps), log L =
    -1/2 (q + log det K) with q = r^T K^-1 r, alpha = K^-1 r, y = L^-1 r.

    Factorisation.  The computed factor is exact for K + dK with |dK| <=
    gamma_{P+1} |L| |L|^T (Higham, Accuracy and Stability of Numerical
    Algorithms, Thm 10.3; the reciprocal of a pivot's root multiplied in
    instead of a division is one more rounding of the P + 1 the theorem
    grants a column).  To first order q moves by -alpha^T dK alpha and log det
    K by tr(K^-1 dK):  1/2 (|alpha|^T |dK| |alpha| + sum_jk |K^-1|_jk
    |dK|_jk).
    Diagonal.  K_jj is a sum of two or three terms >= 0 formed in float64 (C_jj
    + sigma_j^2, or a + (sigma_j^2 + s)): at most two additions, eps K_jj,
    which joins |dK|_jj.
    Forward solve.  Substitution gives (L + dL) y = r with |dL| <= gamma_P
    |L| (Higham Thm 8.5); q = y^T y moves by -2 alpha^T dL y:  gamma_P
    |alpha|^T |L| |y| in log L.
    Sums.  q is a sum of P squares, each rounded, added in a tree or a chain:
    at most P eps q, half of it in log L; the logs of the pivots (1 ulp each)
    and the last additions: eps |log L|.
    Hyper mode.  An off-diagonal K_jk = a rho(D_jk / l) is built in float64.
    In units of u = eps / 2, for the Matern-5/2 function, x = sqrt(5) D (1 /
    l): the constant, 1 / l and two products make x err by 4u of itself; the
    exponential of -x then errs by 4u x e^-x p(x) <= 4.8u with p = 1 + x +
    x^2 / 3 (x p e^-x <= 1.19), and by its own 1 ulp = 2u; the polynomial's
    terms err by 4u x and 11u x^2 / 3 and its two additions by u p each:
    (4 x + 11 x^2 / 3) e^-x <= 3.2u and 2u rho; the product of the two and the
    one with a: 2u.  Together 14u a = 7 eps a; the other three functions have
    fewer operations (the squared exponential: 5u x e^-x <= 1.9u, 2u, u).
    C_B = 8 eps a per element, absolutely, because x e^-x is bounded: an
    argument off by one ulp moves a rho by a fraction of eps a, not of eps
    K_jk.  That is  C_B eps a 1/2 [ (sum_j |alpha_j|)^2 + sum_jk |K^-1|_jk ]."""
    def gamma(k):
        return k * EPS / (1 - k * EPS)

    diag = np.arange(p)
    al = np.abs(ref.alpha)
    ki = np.abs(ref.k_inv)
    dk = gamma(p + 1) * np.einsum('nij,nkj->nik', ref.abs_l, ref.abs_l)
    dk[:, diag, diag] += EPS * ref.k_diag
    tol = 0.5 * (np.einsum('ni,nij,nj->n', al, dk, al) +
                 np.sum(ki * dk, axis=(1, 2)))
    tol += gamma(p) * np.einsum('ni,nij,nj->n', al, ref.abs_l, np.abs(ref.y))
    tol += 0.5 * p * EPS * ref.q + EPS * np.abs(ref.out)
    parts = SimpleNamespace(factorisation=tol.copy())
    if a is not None:
        tol += C_B * EPS * a * 0.5 * (al.sum(axis=1)**2 +
                                      ki.sum(axis=(1, 2)))
    parts.total = tol
    return parts


def case_budget(p, n, mode, kernel, rot=0):
    cov = problem(p, n, mode, kernel, rot)[4]
    return budget(p, expected(p, n, mode, kernel, rot),
                  cov[:, 0] if mode == 'hyper' else None)


def check_classes(p, n, mode, kernel, rot):
    """What a case of ``problem`` holds, checked on the host."""
    t, d, sigma, m, cov = problem(p, n, mode, kernel, rot)
    cls = (np.arange(p) + rot) % 3
    s2 = sigma * sigma
    assert t.shape == ((p, 2) if p == P_2D else (p,))
    assert np.all(np.isfinite(m)) and m.shape == (n, p)
    assert np.array_equal(sigma == 0.0, cls == 0)
    assert np.all((s2[cls == 2] >= 0.01 * (1 - 1e-9)) & (s2[cls == 2] < 0.01002))
    if p >= 15:
        spread = s2[cls == 1]
        assert spread.max() / spread.min() > 1e4
    if mode == 'hyper':
        rcl = np.arange(n) % 4
        assert np.array_equal(cov[:, 0] == 0.0, rcl == 0)
        assert np.all(cov[:, 1:] > 0)
    else:
        assert cov.shape == (n, p, p)
    q = expected(p, n, mode, kernel, rot).q
    assert np.all(q < 3 * p + 30)


# ---------------------------------------------------------------- the twin

@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('p, n, kernel, rot', SHAPES)
def test_twin_stays_inside_the_budget(p, n, kernel, rot, mode):
    """LAPACK in float64 against the long double reference: the reference
    implementation alone must stay inside the bound."""
    check_classes(p, n, mode, kernel, rot)
    t, d, sigma, m, cov = problem(p, n, mode, kernel, rot)
    ref = expected(p, n, mode, kernel, rot)
    tol = case_budget(p, n, mode, kernel, rot)
    got = make(t, d, sigma, mode, kernel).numpy_from_model(m, cov)
    err = np.abs(got - ref.out)
    print('P = %d, n = %d, %s, %s: largest used fraction of the bound %.3g, '
          'of its factorisation part %.3g' % (
              p, n, kernel, mode, (err / tol.total).max(),
              (err / tol.factorisation).max()))
    assert np.all(np.isfinite(got))
    assert np.all(err <= tol.total), (err / tol.total).max()


def _benign(p, n, kernel, seed=0):
    rng = np.random.default_rng(seed)
    t = np.sort(rng.uniform(0, 10, size=p))
    d = rng.normal(size=p)
    sigma = 0.1 + rng.random(p)
    h = np.stack([0.5 + rng.random(n), 0.5 + 2 * rng.random(n),
                  0.01 + 0.1 * rng.random(n)], axis=1)
    m = d + rng.normal(size=(n, p))
    dist = np.abs(t[:, None] - t[None, :])
    k = np.stack([a * gp_correlation(kernel, dist / l) + s * np.eye(p)
                  for a, l, s in h])
    return t, d, sigma, m, h, k


@pytest.mark.parametrize('kernel', GP_KERNELS)
@pytest.mark.parametrize('p', (1, 7, 40))
def test_twin_is_the_multivariate_normal_log_density(p, kernel):
    from scipy.stats import multivariate_normal
    t, d, sigma, m, h, k = _benign(p, 5, kernel)
    like = make(t, d, sigma, 'hyper', kernel, normalised=True)
    assert like.log_norm == -0.5 * p * np.log(2 * np.pi)
    got = like.numpy_from_model(m, h)
    want = [multivariate_normal.logpdf(d, m[i], k[i] + np.diag(sigma**2))
            for i in range(len(m))]
    assert np.all(np.abs(got - want) <= 1e-10 * np.abs(want))
    raw = make(t, d, sigma, 'hyper', kernel).numpy_from_model(m, h)
    assert np.array_equal(raw + like.log_norm, got)


@pytest.mark.parametrize('kernel', GP_KERNELS)
def test_full_mode_with_the_covariance_built_by_hand_equals_hyper_mode(kernel):
    p, n, rot = 49, 17, 1
    t, d, sigma, m, h = problem(p, n, 'hyper', kernel, rot)
    k = make(t, d, None, 'hyper', kernel).numpy_covariance(m, h)
    hyper = make(t, d, sigma, 'hyper', kernel).numpy_from_model(m, h)
    full = make(None, d, sigma, 'full').numpy_from_model(m, k)
    tol = case_budget(p, n, 'hyper', kernel, rot).total
    assert np.all(np.abs(hyper - full) <= 2 * tol)
    # the upper triangle is not read
    k[:, np.triu(np.ones((p, p), bool), 1)] = np.nan
    assert np.array_equal(
        make(None, d, sigma, 'full').numpy_from_model(m, k), full)


def white_noise_problem(p=40, n=9):
    """a = 0, s = 0: independent Gaussians with the quoted error bars."""
    rng = np.random.default_rng(p)
    t = np.sort(rng.uniform(0, 10, size=p))
    d = rng.normal(size=p)
    sigma = 0.1 + rng.random(p)
    m = d + sigma * rng.normal(size=(n, p))
    h = np.tile([0.0, 1.0, 0.0], (n, 1))
    return t, d, sigma, m, h


def fixed_covariance_problem(p=40, n=9):
    """One C for every row, positive definite on its own."""
    t, d, sigma, m, _ = white_noise_problem(p, n)
    rng = np.random.default_rng(p + 1)
    q, _ = np.linalg.qr(rng.normal(size=(p, p)))
    c = (q * 10.0**rng.uniform(-2, 1, size=p)) @ q.T
    c = 0.5 * (c + c.T)
    return d, sigma, m, c


def sum_of_budgets(p, dist, d, sigma, m, cov, mode, kernel='sqexp'):
    """The GP side's budget plus as much again for the other side (the same
    factorisation and solve, done once on the host)."""
    ref = reference(dist, d, sigma, m, cov, mode, kernel)
    return 2 * budget(p, ref, cov[:, 0] if mode == 'hyper' else None).total


def test_white_noise_equals_the_data_vector_likelihood():
    t, d, sigma, m, h = white_noise_problem()
    like = make(t, d, sigma, 'hyper', normalised=True)
    got = like.numpy_from_model(m, h)
    want = GaussianDataLikelihood(identity, d, sigma=sigma).numpy_from_model(m)
    tol = sum_of_budgets(len(d), like.dist, d, sigma, m, h, 'hyper') + \
        4 * EPS * np.abs(want)
    assert np.all(np.abs(got - want) <= tol)


def test_fixed_covariance_equals_the_data_vector_likelihood():
    d, sigma, m, c = fixed_covariance_problem()
    n, p = m.shape
    cov = np.broadcast_to(c, (n, p, p)).copy()
    like = make(None, d, sigma, 'full', normalised=True)
    got = like.numpy_from_model(m, cov)
    want = GaussianDataLikelihood(
        identity, d, cov=c + np.diag(sigma**2)).numpy_from_model(m)
    tol = sum_of_budgets(p, None, d, sigma, m, cov, 'full') + \
        4 * EPS * np.abs(want)
    assert np.all(np.abs(got - want) <= tol)


# ------------------------------------------------- NaN rules, validation

BAD_HYPER = [(0, -1.0), (0, np.nan), (0, np.inf), (1, 0.0), (1, -2.0),
             (1, np.nan), (1, np.inf), (2, -1e-3), (2, np.nan), (2, np.inf)]


def test_nan_rules_of_the_twin():
    t, d, sigma, m, h, k = _benign(12, 8, 'matern32')
    like = make(t, d, sigma, 'hyper', 'matern32')
    good = like.numpy_from_model(m, h)
    assert np.all(np.isfinite(good))
    for col, value in BAD_HYPER:
        hb = h.copy()
        hb[3, col] = value
        out = like.numpy_from_model(m, hb)
        assert np.isnan(out[3]) and np.array_equal(np.delete(out, 3),
                                                   np.delete(good, 3))
    for value in (np.nan, np.inf, -np.inf):
        mb = m.copy()
        mb[5, 7] = value
        out = like.numpy_from_model(mb, h)
        assert np.isnan(out[5]) and np.array_equal(np.delete(out, 5),
                                                   np.delete(good, 5))
    # a = 0 is legal
    hz = h.copy()
    hz[2, 0] = 0.0
    v = sigma**2 + hz[2, 2]
    want = -0.5 * np.sum((m[2] - d)**2 / v + np.log(v))
    assert abs(like.numpy_from_model(m, hz)[2] - want) <= 1e-12 * abs(want)
    full = make(None, d, sigma, 'full')
    good = full.numpy_from_model(m, k)
    kb = k.copy()
    kb[1, 4, 2] = np.nan                       # the lower triangle
    w, v = np.linalg.eigh(k[6])
    w[0] = -1.0
    kb[6] = (v * w) @ v.T - np.diag(sigma**2)  # K itself is indefinite
    out = full.numpy_from_model(m, kb)
    assert np.isnan(out[1]) and np.isnan(out[6])
    keep = np.delete(np.arange(8), [1, 6])
    assert np.array_equal(out[keep], good[keep])


def test_constructor_refuses_bad_arguments():
    t = np.linspace(0, 1, 5)
    d = np.zeros(5)
    with pytest.raises(ValueError, match='model must be callable'):
        GaussianProcessLikelihood(None, t, d)
    with pytest.raises(ValueError, match="cov must be 'hyper' or 'full'"):
        GaussianProcessLikelihood(identity, t, d, cov='diag')
    with pytest.raises(ValueError, match='kernel must be one of'):
        GaussianProcessLikelihood(identity, t, d, kernel='periodic')
    with pytest.raises(ValueError, match="cov='hyper' needs the input"):
        GaussianProcessLikelihood(identity, None, d)
    with pytest.raises(ValueError, match=r't must have shape \(5,\) or '):
        GaussianProcessLikelihood(identity, t[:4], d)
    with pytest.raises(ValueError, match='t must have shape'):
        GaussianProcessLikelihood(identity, np.zeros((5, 2, 2)), d)
    with pytest.raises(ValueError, match='t must be finite'):
        GaussianProcessLikelihood(identity, np.full(5, np.nan), d)
    with pytest.raises(ValueError, match='data must be a vector'):
        GaussianProcessLikelihood(identity, t, np.zeros((5, 1)))
    with pytest.raises(ValueError, match='data must be finite'):
        GaussianProcessLikelihood(identity, t, np.full(5, np.inf))
    with pytest.raises(ValueError, match='at most 128 data points'):
        GaussianProcessLikelihood(identity, np.zeros(129), np.zeros(129))
    with pytest.raises(ValueError, match='sigma must be 5 finite numbers '
                                         'that are not negative'):
        GaussianProcessLikelihood(identity, t, d, -np.ones(5))
    with pytest.raises(ValueError, match='sigma must be 5'):
        GaussianProcessLikelihood(identity, t, d, np.ones(4))
    assert N_GP_MAX == 128
    like = GaussianProcessLikelihood(identity, np.zeros((128, 3)),
                                     np.zeros(128), cov='full')
    assert like.n_data == 128 and like.dist.shape == (128, 128)
    assert GaussianProcessLikelihood(identity, None, d, cov='full').dist is None


def test_model_outputs_are_checked():
    t = np.linspace(0, 1, 5)
    like = make(t, np.zeros(5), None, 'hyper')
    m, h = np.zeros((3, 5)), np.ones((3, 3))
    with pytest.raises(ValueError, match='must be float64, not float32'):
        like.from_model(m.astype(np.float32), h)
    with pytest.raises(ValueError, match='must be float64, not float32'):
        like.from_model(m, h.astype(np.float32))
    with pytest.raises(ValueError, match='must be float64'):
        like.from_model(torch.zeros(3, 5), torch.ones(3, 3,
                                                      dtype=torch.float64))
    with pytest.raises(ValueError, match=r'shape \(n, 5\)'):
        like.from_model(np.zeros((3, 4)), h)
    with pytest.raises(ValueError, match=r'covariance input must have shape '
                                         r'\(3, 3\)'):
        like.from_model(m, np.ones((3, 4)))
    with pytest.raises(ValueError, match='both be torch tensors or both'):
        like.from_model(torch.from_numpy(m), h)
    full = make(None, np.zeros(5), None, 'full')
    with pytest.raises(ValueError, match=r'covariance input must have shape '
                                         r'\(3, 5, 5\)'):
        full.from_model(m, np.ones((3, 25)))
    with pytest.raises(ValueError, match=r'covariance input must have shape '
                                         r'\(3, 5, 5\)'):
        full.from_model(m, np.ones((2, 5, 5)))


def pair_model(x):
    return x[:, :4], x[:, 4:7] + 1.0


def test_pickle_round_trip_and_numpy_call():
    t = np.linspace(0, 3, 4)
    like = GaussianProcessLikelihood(pair_model, t, np.full(4, 0.5),
                                     np.full(4, 0.1), kernel='exp')
    like._tables['fake'] = object()
    again = pickle.loads(pickle.dumps(like))
    assert again._tables == {} and again.kernel == 'exp'
    assert np.array_equal(again.dist, like.dist)
    x = np.random.default_rng(0).random((6, 7))
    want = like.numpy_from_model(x[:, :4], x[:, 4:7] + 1.0)
    assert np.array_equal(again.numpy(x), want)
    assert np.all(np.isfinite(want))


def test_exported_lazily():
    import nautilus_amd
    assert 'GaussianProcessLikelihood' in nautilus_amd.__all__
    assert nautilus_amd.GaussianProcessLikelihood is GaussianProcessLikelihood
