"""The fused device likelihood of a Gaussian data vector (``nb_chi2_loglike``,
nautilus_amd/csrc/nb_chi2.hip) against a long-double reference under a
derived error bound, its bit-for-bit independence of the batch, and end to
end through ``Sampler``."""

import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

RTOL, ATOL = 1e-11, 1e-8          # the band tests/test_hip_parity.py holds the
#                                   likelihoods to
EPS = 2.0**-52

# the smallest shapes that cross each boundary of the kernel: one k-step, one
# tile, one wavefront's row tiles (128), one panel (256), several panels, the
# largest P
SHAPES = [(p, 530) for p in (1, 3, 16, 17, 64, 65, 128, 129, 200, 257)] + \
    [(p, 67) for p in (1000, 1025, 2049)] + [(4096, 33)]
SIGMA_SHAPES = [(1, 530), (17, 530), (129, 530), (4096, 33)]


def identity(x):
    return x


@functools.lru_cache(maxsize=None)
def problem(p, n):
    """data, C = 1e-2 (A A^T / K + 0.5 I) with A a (P, K) standard normal
    matrix, W = L^-1 of its Cholesky factor, and n model rows: half near the
    data (|r| ~ sigma), half far (|r| ~ 1e3 sigma).  K = P up to P = 257, the
    recipe of test_data_likelihood.py; K = 256 beyond (C and W stay dense,
    building them stays cheap).  Computed once per shape; nobody writes to
    it."""
    from scipy.linalg import lapack, solve_triangular
    rng = np.random.default_rng(1000 * p + n)
    k = p if p <= 257 else 256
    a = rng.normal(size=(p, k))
    cov = 1e-2 * (a @ a.T / k + 0.5 * np.eye(p))
    cov = 0.5 * (cov + cov.T)
    d = rng.normal(size=p)
    sigma = np.sqrt(np.diag(cov))
    scale = np.where(np.arange(n) % 2 == 0, 1.0, 1e3)[:, None]
    m = d + scale * sigma * rng.normal(size=(n, p))
    chol = np.linalg.cholesky(cov)
    if p <= 257:
        # the recipe of GaussianDataLikelihood: the class and a table built
        # from this W give the same bits
        w = np.tril(solve_triangular(chol, np.eye(p), lower=True))
    else:
        w, info = lapack.dtrtri(chol, lower=1)
        assert info == 0
        w = np.tril(w)
    for arr in (d, cov, sigma, m, w):
        arr.setflags(write=False)
    return d, cov, sigma, m, w


def reference(w, d, m):
    """chi^2 in long double from the same W, data and model, and the bound
    4 (P + 2) eps sum_j ((|W| |r|)_j)^2 on the error of an fp64 evaluation: a
    length-P dot product errs by at most gamma_P (|W| |r|)_j, squaring and
    summing add 2 gamma_P + gamma_P, the residual subtraction adds eps.  (The
    long-double product skips the zeros above the diagonal of W, 256 rows at
    a time; the magnitudes of the bound are a sum of positive terms, for
    which fp64 is ample.)"""
    assert np.finfo(np.longdouble).eps < 1e-18
    ld = np.longdouble
    p = w.shape[0]
    r = m.astype(ld) - d.astype(ld)
    if w.ndim == 1:                              # the diagonal of a diagonal W
        y = r * w.astype(ld)
        mag = np.abs(np.asarray(r, float)) * w
    else:
        wl = w.astype(ld)
        y = np.empty(r.shape, ld)
        for j in range(0, p, 256):
            e = min(j + 256, p)
            y[:, j:e] = (wl[j:e, :e] @ np.ascontiguousarray(r[:, :e].T)).T
        mag = np.abs(np.asarray(r, float)) @ np.abs(w).T
    chi2 = np.sum(y * y, axis=1)
    bound = 4 * (p + 2) * EPS * np.sum(mag * mag, axis=1)
    return chi2, bound


def _check(out, chi2, bound, log_norm=0.0, what=''):
    """-2 (out - log_norm) against the long-double chi^2."""
    ld = np.longdouble
    got = -2 * (out.astype(ld) - ld(log_norm))
    extra = 0.0
    if log_norm != 0.0:
        # forming log_norm - chi2 / 2 rounds once more; in units of chi^2
        extra = 2 * (2 * EPS * np.maximum(abs(log_norm), np.abs(out)))
    used = np.abs(got - chi2) / (bound + extra)
    print('%s: largest used fraction of the bound %.3g' % (what, used.max()))
    assert np.all(np.isfinite(out))
    assert np.all(used <= 1.0), (what, used.max())


@pytest.mark.parametrize('p, n', SHAPES)
def test_values_full_covariance(p, n):
    import torch
    from nautilus_amd import GaussianDataLikelihood
    d, cov, _, m, w = problem(p, n)
    chi2, bound = reference(w, d, m)
    like = GaussianDataLikelihood(identity, d, cov=cov, normalised=False)
    # the handle gets the very W of the reference
    from nautilus_amd import device
    table = device.Chi2Table(d, chol_inv=w)
    mt = torch.from_numpy(m).cuda()
    out = table.loglike(mt)
    assert out.is_cuda and out.dtype == torch.float64 and out.shape == (n,)
    _check(out.cpu().numpy(), chi2, bound, what='P = %d, table' % p)
    got = out.cpu().numpy()
    if p <= 257:
        # the class derives the same W from cov (problem() repeats its recipe)
        assert torch.equal(like.from_model(mt), out)
        twin = like.numpy_from_model(m)
        err = np.abs(got - twin) / (ATOL + RTOL * np.abs(twin))
        print('numpy twin: largest error %.3g of the band' % err.max())
        assert np.allclose(got, twin, rtol=RTOL, atol=ATOL)
    # normalised: the constant is added with one more rounding
    log_norm = GaussianDataLikelihood(identity, d, cov=cov).log_norm
    table = device.Chi2Table(d, chol_inv=w, log_norm=log_norm)
    _check(table.loglike(mt).cpu().numpy(), chi2, bound, log_norm,
           what='P = %d, normalised' % p)


@pytest.mark.parametrize('p, n', SIGMA_SHAPES)
def test_values_sigma(p, n):
    import torch
    from nautilus_amd import GaussianDataLikelihood, device
    d, _, sigma, m, _ = problem(p, n)
    inv = 1.0 / sigma
    chi2, bound = reference(inv, d, m)
    mt = torch.from_numpy(m).cuda()
    out = device.Chi2Table(d, inv_sigma=inv).loglike(mt)
    assert out.is_cuda and out.dtype == torch.float64 and out.shape == (n,)
    _check(out.cpu().numpy(), chi2, bound, what='P = %d, sigma' % p)
    like = GaussianDataLikelihood(identity, d, sigma=sigma)
    got = like.from_model(mt).cpu().numpy()
    if p <= 257:
        assert np.allclose(got, like.numpy_from_model(m), rtol=RTOL,
                           atol=ATOL)
    table = device.Chi2Table(d, inv_sigma=inv, log_norm=like.log_norm)
    _check(table.loglike(mt).cpu().numpy(), chi2, bound, like.log_norm,
           what='P = %d, sigma, normalised' % p)


@pytest.mark.parametrize('p', [3, 129, 257, 1025])
@pytest.mark.parametrize('diag', [False, True], ids=['cov', 'sigma'])
def test_ragged_batches_bit_for_bit(p, diag):
    """Any slice of a batch, taken at an odd row offset, gives the bits the
    same rows have inside the large batch; so does a column slice of a wider
    tensor, read in place."""
    import torch
    from nautilus_amd import GaussianDataLikelihood, device
    d, cov, sigma, _, w = problem(p, 67 if p > 257 else 530)
    rng = np.random.default_rng(p)
    big = torch.from_numpy(d + 30 * sigma * rng.normal(size=(2000, p))).cuda()
    kw = dict(sigma=sigma) if diag else dict(cov=cov)
    like = GaussianDataLikelihood(identity, d, **kw)
    full = like.from_model(big)
    assert bool(torch.isfinite(full).all())
    for n in (0, 1, 15, 16, 17, 63, 65, 1000):
        for off in (1, 777):
            sub = big[off:off + n]
            if n > 0:                   # a view, not a copy
                assert sub.data_ptr() == big.data_ptr() + off * p * 8
            out = like.from_model(sub)
            assert out.shape == (n,)
            assert torch.equal(out, full[off:off + n]), (n, off)
    # a column slice of a wider tensor: rows P + 11 doubles apart
    wide = torch.from_numpy(rng.normal(size=(2000, p + 11))).cuda()
    wide[:, 5:5 + p] = big
    view = wide[:, 5:5 + p]
    assert view.data_ptr() == wide.data_ptr() + 5 * 8
    assert view.stride() == (p + 11, 1)
    assert torch.equal(like.from_model(view), full)
    # ... handed to the table as it is, with ld = P + 11: no copy anywhere
    table = like._table()
    assert torch.equal(table.loglike(view, ld=p + 11), full)
    assert torch.equal(table.loglike(view), full)
    # the launcher picks larger blocks of points for larger batches
    if not diag and p <= 129:
        reps = torch.cat([big] * 17)                    # 34 000 rows
        assert torch.equal(like.from_model(reps), torch.cat([full] * 17))
        assert torch.equal(like.from_model(reps[:20000]),
                           torch.cat([full] * 10))
    # ... and walks a second panel of W with them: 32 768 rows are the first
    # batch of the largest block, 16 384 of the middle one
    if not diag and p == 257:
        reps = torch.cat([big] * 17)[:32768]
        want = torch.cat([full] * 17)[:32768]
        assert torch.equal(like.from_model(reps), want)
        assert torch.equal(like.from_model(reps[:16384]), want[:16384])


@pytest.mark.parametrize('p', [17, 129])
@pytest.mark.parametrize('diag', [False, True], ids=['cov', 'sigma'])
def test_nan_stays_in_its_row(p, diag):
    import torch
    from nautilus_amd import GaussianDataLikelihood
    d, cov, sigma, m, _ = problem(p, 530)
    kw = dict(sigma=sigma) if diag else dict(cov=cov)
    like = GaussianDataLikelihood(identity, d, **kw)
    clean = torch.from_numpy(m[:40].copy()).cuda()
    want = like.from_model(clean)
    keep = torch.ones(40, dtype=torch.bool, device='cuda')
    keep[5] = keep[19] = False
    # +inf in the first column of a k-tile meets no exact zero of W in its
    # own row tile; in any other column it does: both must give NaN
    for c_nan, c_inf in ((2, 0), (p - 1, 16), (0, p - 1)):
        dirty = clean.clone()
        dirty[5, c_nan] = float('nan')
        dirty[19, c_inf] = float('inf')
        out = like.from_model(dirty)
        assert bool(torch.isnan(out[5])) and bool(torch.isnan(out[19]))
        assert torch.equal(out[keep], want[keep])
    dirty = clean.clone()
    dirty[19, 3] = float('-inf')
    out = like.from_model(dirty)
    assert bool(torch.isnan(out[19]))
    keep[5] = True
    assert torch.equal(out[keep], want[keep])


def test_one_handle_on_two_streams():
    import torch
    from nautilus_amd import GaussianDataLikelihood
    d, cov, _, m, _ = problem(200, 530)
    like = GaussianDataLikelihood(identity, d, cov=cov)
    x = torch.from_numpy(m).cuda()
    want = like(x)
    torch.cuda.synchronize()
    outs = []
    for s in (torch.cuda.Stream(), torch.cuda.Stream()):
        with torch.cuda.stream(s):
            outs.append(like(x))
    torch.cuda.synchronize()
    assert like._tables and len(like._tables) == 1
    assert list(like._tables) == [torch.cuda.current_device()]
    assert torch.equal(outs[0], want) and torch.equal(outs[1], want)


def test_argument_errors_carry_err_arg():
    import torch
    from nautilus_amd import _lib, device

    def code(*args, **kw):
        with pytest.raises(_lib.NativeError) as err:
            device.Chi2Table(*args, **kw)
        return err.value.code

    d = np.full(3, 0.5)
    eye = np.eye(3)
    one = np.ones(3)
    assert device.Chi2Table(d, chol_inv=eye).n_data == 3
    assert device.Chi2Table(d, inv_sigma=one).n_data == 3
    # n_data outside 1 .. 4096
    assert code(np.zeros(0), inv_sigma=np.zeros(0)) == _lib.ERR_ARG
    assert code(np.zeros(4097), inv_sigma=np.ones(4097)) == _lib.ERR_ARG
    assert device.Chi2Table(np.zeros(4096),
                            inv_sigma=np.ones(4096)).n_data == 4096
    # both, neither
    assert code(d, chol_inv=eye, inv_sigma=one) == _lib.ERR_ARG
    assert code(d) == _lib.ERR_ARG
    # non-finite inputs
    assert code(d * np.nan, chol_inv=eye) == _lib.ERR_ARG
    assert code(np.r_[0.5, np.inf, 0.5], inv_sigma=one) == _lib.ERR_ARG
    assert code(d, chol_inv=np.where(eye > 0, np.inf, 0.0)) == _lib.ERR_ARG
    assert code(d, inv_sigma=np.r_[1.0, np.nan, 1.0]) == _lib.ERR_ARG
    assert code(d, inv_sigma=np.r_[1.0, np.inf, 1.0]) == _lib.ERR_ARG
    assert code(d, chol_inv=eye, log_norm=np.nan) == _lib.ERR_ARG
    bad = eye.copy()
    bad[2, 1] = np.nan                                  # below the diagonal
    assert code(d, chol_inv=bad) == _lib.ERR_ARG
    bad = eye.copy()
    bad[0, 2] = 1e-3                                    # above the diagonal
    assert code(d, chol_inv=bad) == _lib.ERR_ARG
    # a non-positive diagonal entry
    bad = eye.copy()
    bad[1, 1] = 0.0
    assert code(d, chol_inv=bad) == _lib.ERR_ARG
    bad[1, 1] = -1.0
    assert code(d, chol_inv=bad) == _lib.ERR_ARG
    assert code(d, inv_sigma=np.r_[1.0, 0.0, 1.0]) == _lib.ERR_ARG
    assert code(d, inv_sigma=np.r_[1.0, -1.0, 1.0]) == _lib.ERR_ARG
    # ld < n_data
    table = device.Chi2Table(d, chol_inv=eye)
    m = torch.zeros(4, 3, dtype=torch.float64, device='cuda')
    with pytest.raises(_lib.NativeError) as err:
        table.loglike(m, ld=2)
    assert err.value.code == _lib.ERR_ARG
    assert table.loglike(m, ld=3).shape == (4,)
    # shapes that do not fit together never reach the library
    with pytest.raises(ValueError):
        device.Chi2Table(d, chol_inv=np.eye(4))
    with pytest.raises(ValueError):
        device.Chi2Table(d, inv_sigma=np.ones(4))


def test_model_output_validation():
    import torch
    from nautilus_amd import GaussianDataLikelihood
    d, cov, _, m, _ = problem(17, 530)
    like = GaussianDataLikelihood(identity, d, cov=cov)
    mt = torch.from_numpy(m).cuda()
    with pytest.raises(ValueError):
        like.from_model(mt[:, :16])
    with pytest.raises(ValueError):
        like.from_model(mt[0])
    with pytest.raises(ValueError):
        like.from_model(mt.float())
    # anything but unit-stride rows is copied, and gives the same bits
    want = like.from_model(mt)
    assert torch.equal(like.from_model(mt.t().contiguous().t()), want)
    twice = torch.stack([mt, mt], dim=2)[:, :, 0]       # stride(1) == 2
    assert twice.stride(1) == 2
    assert torch.equal(like.from_model(twice), want)


def test_numpy_in_numpy_out():
    import torch
    from nautilus_amd import GaussianDataLikelihood
    rng = np.random.default_rng(8)
    d, cov, sigma, _, _ = problem(65, 530)
    a = rng.normal(size=(65, 4))
    a_dev = {}

    def model(x):
        if x.device not in a_dev:
            a_dev[x.device] = torch.from_numpy(a).to(x.device)
        return x @ a_dev[x.device].T

    x = rng.random((333, 4))
    for kw in (dict(cov=cov), dict(sigma=sigma)):
        like = GaussianDataLikelihood(model, d, **kw)
        out = like(x)
        assert isinstance(out, np.ndarray) and out.shape == (333,)
        t_out = like(torch.from_numpy(x).cuda())
        assert t_out.is_cuda
        assert np.array_equal(out, t_out.cpu().numpy())
        m = (torch.from_numpy(x) @ torch.from_numpy(a).T).numpy()
        m_out = like.from_model(m)
        assert isinstance(m_out, np.ndarray)
        assert np.allclose(m_out, like.numpy(x), rtol=RTOL, atol=ATOL)


@functools.lru_cache(maxsize=None)
def _linear_problem():
    """P = 200 data points linear in three parameters: data = A theta_0, a
    full covariance scaled so that every posterior standard deviation is
    between 0.02 and 0.04 (the faces of the cube are >= 10 sigma away)."""
    rng = np.random.default_rng(12)
    p = 200
    a = rng.normal(size=(p, 3))
    theta0 = np.array([0.4, 0.5, 0.6])
    b = rng.normal(size=(p, p))
    cov = b @ b.T / p + 0.5 * np.eye(p)
    post = np.linalg.inv(a.T @ np.linalg.solve(cov, a))
    cov *= 0.03**2 / np.sqrt(np.diag(post)).mean()**2
    cov = 0.5 * (cov + cov.T)
    post = np.linalg.inv(a.T @ np.linalg.solve(cov, a))
    sd = np.sqrt(np.diag(post))
    assert np.all(sd > 0.02) and np.all(sd < 0.04), sd
    return a, theta0, a @ theta0, cov, post


def _run_linear():
    import torch
    from nautilus_amd import GaussianDataLikelihood, Sampler, unit_prior
    a, _, data, cov, _ = _linear_problem()
    a_dev = torch.from_numpy(a).cuda()
    like = GaussianDataLikelihood(lambda x: x @ a_dev.T, data, cov=cov)
    s = Sampler(unit_prior, like, n_dim=3, n_live=1000, n_networks=2,
                vectorized=True, seed=1, n_batch=1000)
    s.run(n_eff=5000, discard_exploration=True)
    return like, s


def test_sampler_recovers_linear_model():
    """Evidence and posterior mean of a linear model in the settings and the
    evidence band of test_sampler_recovers_unequal_mode_weights: the
    posterior is the Gaussian N(theta_0, Sigma_post), Sigma_post = (A^T C^-1
    A)^-1, so log Z = log_norm + 1/2 log det(2 pi Sigma_post)."""
    _, theta0, _, _, post = _linear_problem()
    like, s = _run_linear()
    analytic = like.log_norm + 0.5 * np.linalg.slogdet(2 * np.pi * post)[1]
    print('log Z = %.4f, analytic %.4f, n_like = %d, n_eff = %.0f' % (
        s.log_z, analytic, s.n_like, s.n_eff))
    assert abs(s.log_z - analytic) < 0.06
    pts, log_w, _ = s.posterior()
    wgt = np.exp(log_w - np.max(log_w))
    mean = wgt @ pts / wgt.sum()
    tol = 4 * np.sqrt(np.diag(post)) / np.sqrt(s.n_eff)
    print('posterior mean - theta_0 in units of the tolerance:',
          (mean - theta0) / tol)
    assert np.all(np.abs(mean - theta0) < tol)
    _, again = _run_linear()
    assert again.log_z == s.log_z and again.n_like == s.n_like
