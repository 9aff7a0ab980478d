"""The fused device Gaussian likelihood with per-point noise parameters
(``nb_noise_loglike``, nautilus_amd/csrc/nb_noise.hip) against the defining
formula in ``np.longdouble`` under a derived error bound, its bit-for-bit
independence of the batch, its NaN rules, and end to end through ``Sampler``.
The problems, the reference and the bound (``budget``, with its derivation)
live in test_noise_likelihood.py, which holds the numpy twin to them without
a GPU."""

import functools

import numpy as np
import pytest

from test_noise_likelihood import (EDGE_TEST_P, EPS, LONG_SHAPES, MODES,
                                   ROW_TEST_P, SHAPES, budget, check_classes,
                                   expected, identity, long_expected,
                                   long_problem, make, problem, reference,
                                   unit_inflation_problem,
                                   zero_residual_problem)

pytestmark = pytest.mark.gpu


def _mode(mode):
    from nautilus_amd import device
    return device.NOISE_ROW if mode == 'row' else device.NOISE_FULL


def test_shapes_cover_both_sides_of_every_launcher_boundary():
    from nautilus_amd import device
    ps = sorted({s[0] for s in SHAPES})
    shapes = [device.noise_launch_shape(p) for p in range(1, 5000)]
    changes = [p for p in range(1, 4999) if shapes[p - 1] != shapes[p]]
    assert changes == [32, 512]
    for p in changes:
        assert p in ps and p + 1 in ps


@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('p, n, rot', SHAPES)
def test_values(p, n, rot, mode):
    """|device - long double| <= budget(P, X, A) in every row (the budget is
    derived in test_noise_likelihood.budget)."""
    import torch
    check_classes(p, n, mode, rot)
    d, sigma, m, w = problem(p, n, mode, rot)
    want, x, a, _, _ = expected(p, n, mode, rot)
    tol = budget(p, x, a)
    raw = make(d, sigma, mode)
    mt, wt = torch.from_numpy(m).cuda(), torch.from_numpy(w).cuda()
    out = raw.from_model(mt, wt)
    assert out.is_cuda and out.dtype == torch.float64 and out.shape == (n,)
    got = out.cpu().numpy()
    used = np.abs(got - want) / tol
    print('P = %d, n = %d, rot = %d, %s: largest used fraction of the bound '
          '%.3g' % (p, n, rot, mode, used.max()))
    assert np.all(np.isfinite(got))
    assert np.all(np.abs(got - want) <= tol), used.max()
    # the constant joins with one subtraction: log_norm - sum / 2
    like = make(d, sigma, mode, normalised=True)
    assert like.log_norm == -0.5 * p * np.log(2 * np.pi)
    assert np.array_equal(like.from_model(mt, wt).cpu().numpy(),
                          like.log_norm + got)


@pytest.mark.parametrize('p, n', LONG_SHAPES)
def test_long_rows(p, n):
    """Every v in [1, 1.001): each mantissa is about 1/2, and a running
    product that is not renormalised underflows (LONG_SHAPES says where)."""
    import torch
    d, sigma, m, w = long_problem(p, n)
    want, x, a, v_min, v_max = long_expected(p, n)
    assert 1.0 <= v_min and v_max < 1.001
    tol = budget(p, x, a)
    out = make(d, sigma, 'row').from_model(torch.from_numpy(m).cuda(),
                                           torch.from_numpy(w).cuda())
    got = out.cpu().numpy()
    used = np.abs(got - want) / tol
    print('P = %d, n = %d: largest used fraction of the bound %.3g' % (
        p, n, used.max()))
    assert np.all(np.isfinite(got))
    assert np.all(np.abs(got - want) <= tol), used.max()


@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('p', ROW_TEST_P)
def test_rows_bit_for_bit(p, mode):
    """A row's bits are those it has alone, inside batches of 17 and 4097 at
    different positions, with m and w each in place inside a wider tensor, on
    any stream."""
    import torch
    d, sigma, m, w = problem(p, 4097, mode)
    like = make(d, sigma, mode, normalised=True)
    width = w.shape[1]
    big, noise = torch.from_numpy(m).cuda(), torch.from_numpy(w).cuda()
    full = like.from_model(big, noise)
    assert bool(torch.isfinite(full).all())
    for off in (0, 1, 777, 4080):
        sub, wsub = big[off:off + 17], noise[off:off + 17]
        assert sub.data_ptr() == big.data_ptr() + off * p * 8   # a view
        assert wsub.data_ptr() == noise.data_ptr() + off * width * 8
        assert torch.equal(like.from_model(sub, wsub), full[off:off + 17]), off
        for r in (off, off + 16):
            assert torch.equal(like.from_model(big[r:r + 1], noise[r:r + 1]),
                               full[r:r + 1])
    # the same rows at other positions of a batch
    perm = torch.from_numpy(np.random.default_rng(p).permutation(4097)).cuda()
    assert torch.equal(like.from_model(big[perm], noise[perm]), full[perm])
    assert like.from_model(big[:0], noise[:0]).shape == (0,)
    # column slices of wider tensors, m and w independently
    rng = np.random.default_rng(p)
    wide = torch.from_numpy(rng.normal(size=(4097, p + 5))).cuda()
    wide[:, 2:2 + p] = big
    view = wide[:, 2:2 + p]
    assert view.data_ptr() == wide.data_ptr() + 2 * 8
    assert view.stride() == (p + 5, 1)
    wwide = torch.from_numpy(rng.normal(size=(4097, width + 3))).cuda()
    wwide[:, 1:1 + width] = noise
    wview = wwide[:, 1:1 + width]
    assert wview.data_ptr() == wwide.data_ptr() + 8
    assert wview.stride() == (width + 3, 1)
    assert torch.equal(like.from_model(view, noise), full)
    assert torch.equal(like.from_model(big, wview), full)
    assert torch.equal(like.from_model(view, wview), full)
    table = like._table()
    code = _mode(mode)
    assert torch.equal(table.loglike(view, wview, code, ld=p + 5,
                                     ld_noise=width + 3), full)
    assert torch.equal(table.loglike(view[5:22], wview[5:22], code),
                       full[5:22])
    assert torch.equal(table.loglike(view[40:41], noise[40:41], code),
                       full[40:41])
    # a stream of its own
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        other = like.from_model(big, noise)
        one = like.from_model(view[9:10], wview[9:10])
    stream.synchronize()
    assert torch.equal(other, full) and torch.equal(one, full[9:10])


@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('p', EDGE_TEST_P)
def test_edge_rows(p, mode):
    import torch
    d, sigma, m, w = problem(p, 1000, mode)
    like = make(d, sigma, mode, normalised=True)
    cm = torch.from_numpy(m[:100].copy()).cuda()
    cw = torch.from_numpy(w[:100].copy()).cuda()
    want = like.from_model(cm, cw)
    assert bool(torch.isfinite(want).all())
    cls = np.arange(p) % 4
    c_zero = int(np.flatnonzero(cls == 0)[-1])          # sigma_j = 0
    c_one = int(np.flatnonzero(cls == 2)[0])            # sigma_j^2 ~ 1
    c_last = p - 1
    assert sigma[c_zero] == 0 and sigma[c_one] >= 1
    dm, dw = cm.clone(), cw.clone()
    dm[40, 0] = float('nan')
    dm[41, c_last] = float('inf')
    dm[42, 1] = float('-inf')
    if mode == 'row':
        dw[3] = torch.tensor([1.0, 0.0, 0.0])           # v = 0 at sigma_j = 0
        dw[11] = torch.tensor([1.0, -2.0, 0.0])         # v < 0 at sigma^2 ~ 1
        dw[12, 1] = float('inf')                        # a = +inf
        dw[13, 0] = float('nan')
        dw[14, 2] = float('nan')
        dw[77] = torch.tensor([0.0, 0.0, 0.0])          # v = 0 everywhere
        dw[99, 1] = float('-inf')
        bad = [3, 11, 12, 13, 14, 40, 41, 42, 77, 99]
    else:
        dw[3, c_zero] = 0.0                             # v = 0
        dw[11, c_one] = -2.0                            # v < 0
        dw[12, c_last] = float('inf')
        dw[13, 0] = float('nan')
        dw[14, c_last] = float('nan')
        dw[77, c_zero] = -1e-300
        dw[99, c_one] = float('-inf')
        bad = [3, 11, 12, 13, 14, 40, 41, 42, 77, 99]
    out = like.from_model(dm, dw)
    for i in bad:
        assert bool(torch.isnan(out[i])), i
    keep = torch.ones(100, dtype=torch.bool, device='cuda')
    keep[bad] = False
    assert torch.equal(out[keep], want[keep])
    twin = like.numpy_from_model(dm.cpu().numpy(), dw.cpu().numpy())
    assert np.array_equal(np.isnan(twin), torch.isnan(out).cpu().numpy())
    # the sign of a single coefficient does not matter while v > 0
    sm, sw = cm[5:6].clone(), cw[5:6].clone()
    if mode == 'row':
        sw[0] = torch.tensor([-1e-13, float(sigma.max()**2) + 1.0, 0.5])
    else:
        sw[0, c_one] = -0.5
    got = like.from_model(sm, sw)
    assert bool(torch.isfinite(got).all())
    assert np.isfinite(like.numpy_from_model(sm.cpu().numpy(),
                                             sw.cpu().numpy())[0])
    # r = 0 with v > 0: a finite row within the budget
    zd, zs, zm, zw = zero_residual_problem(p, mode)
    ref, x, a, v_min, _ = reference(zd, zs, zm, zw, mode)
    assert x[0] == 0.0 and v_min > 0
    got = float(make(zd, zs, mode).from_model(
        torch.from_numpy(zm).cuda(), torch.from_numpy(zw).cuda())[0])
    assert np.isfinite(got) and abs(got - ref[0]) <= budget(p, x, a)[0]


def test_one_handle_on_two_streams():
    import torch
    d, sigma, m, w = problem(257, 1000, 'row')
    wt = torch.from_numpy(w).cuda()
    from nautilus_amd import GaussianNoiseLikelihood
    like = GaussianNoiseLikelihood(lambda x: (x, wt), d, sigma)
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
    import ctypes
    import torch
    from nautilus_amd import _lib, device

    def code(*args, **kw):
        with pytest.raises(_lib.NativeError) as err:
            device.NoiseTable(*args, **kw)
        assert str(err.value) != 'nautilus_hip: '
        return err.value.code

    d = np.array([0.5, -2.0, 5.5])
    assert device.NoiseTable(d).n_data == 3
    assert device.NoiseTable(d, np.r_[0.0, 1.0, 4.0], log_norm=-3.0).n_data \
        == 3
    # n_data outside 1 .. 2^20
    assert code(np.zeros(0)) == _lib.ERR_ARG
    assert code(np.zeros((1 << 20) + 1)) == _lib.ERR_ARG
    assert device.NoiseTable(np.zeros(1 << 20)).n_data == 1 << 20
    # data, sigma2, constant
    assert code(np.r_[1.0, np.nan, 1.0]) == _lib.ERR_ARG
    assert code(np.r_[1.0, -np.inf, 1.0]) == _lib.ERR_ARG
    for bad in (-1e-300, np.nan, np.inf):
        assert code(d, np.r_[0.0, bad, 1.0]) == _lib.ERR_ARG
    assert code(d, log_norm=np.nan) == _lib.ERR_ARG
    assert code(d, log_norm=np.inf) == _lib.ERR_ARG
    # NULL data, NULL out
    lib = _lib.load()
    h = ctypes.c_void_p()

    def raw_refused(fn, *args):
        # another entry's message first: the text checked below is this call's
        assert lib.nb_poisson_create(0, None, None, None, 0.0,
                                     None) == _lib.ERR_ARG
        assert b'Poisson' in lib.nb_last_error()
        assert fn(*args) == _lib.ERR_ARG
        assert b'noise likelihood' in lib.nb_last_error()

    raw_refused(lib.nb_noise_create, 3, None, None, 0.0, ctypes.byref(h))
    raw_refused(lib.nb_noise_create, 3, d.ctypes.data_as(_lib.c_double_p),
                None, 0.0, None)
    table = device.NoiseTable(d, np.ones(3))
    m = torch.ones(4, 3, dtype=torch.float64, device='cuda')
    w3 = torch.ones(4, 3, dtype=torch.float64, device='cuda')
    row, full = device.NOISE_ROW, device.NOISE_FULL

    def refused(*args, **kw):
        with pytest.raises(_lib.NativeError) as err:
            table.loglike(*args, **kw)
        assert err.value.code == _lib.ERR_ARG and str(err.value)

    # an unknown mode
    refused(m, w3, 2)
    refused(m, w3, -1)
    # ld and ld_noise count from the second row on
    refused(m, w3, row, ld=2)
    refused(m, w3, row, ld_noise=2)
    refused(m, w3, full, ld_noise=2)
    refused(m, w3, full, ld=2)
    want = table.loglike(m, w3, row)
    assert want.shape == (4,)
    assert torch.equal(table.loglike(m, w3, row, ld=3, ld_noise=3), want)
    assert torch.equal(table.loglike(m[:1], w3[:1], row, ld=0, ld_noise=0),
                       want[:1])
    assert torch.equal(table.loglike(m[:1], w3[:1], full, ld=0, ld_noise=0),
                       table.loglike(m, w3, full)[:1])
    # row mode with P = 1 still needs three doubles of noise per row
    one = device.NoiseTable(np.zeros(1), np.ones(1))
    m1 = torch.ones(4, 1, dtype=torch.float64, device='cuda')
    with pytest.raises(_lib.NativeError):
        one.loglike(m1, w3, row, ld_noise=1)
    assert one.loglike(m1, w3, row).shape == (4,)
    assert one.loglike(m1, m1, full, ld_noise=1).shape == (4,)
    # NULL pointers with n > 0, and none needed for n = 0
    out = torch.empty(4, dtype=torch.float64, device='cuda')
    ptrs = dict(h=table._h, m=m.data_ptr(), w=w3.data_ptr(),
                out=out.data_ptr())
    for null in ('h', 'm', 'w', 'out'):
        a = dict(ptrs)
        a[null] = None
        raw_refused(lib.nb_noise_loglike, a['h'], row, a['m'], 3, a['w'], 3,
                    4, a['out'], None)
    raw_refused(lib.nb_noise_loglike, table._h, row, m.data_ptr(), 3,
                w3.data_ptr(), 3, -1, out.data_ptr(), None)
    raw_refused(lib.nb_noise_loglike, table._h, 7, m.data_ptr(), 3,
                w3.data_ptr(), 3, 4, out.data_ptr(), None)
    assert lib.nb_noise_loglike(table._h, row, None, 3, None, 3, 0, None,
                                None) == 0
    assert lib.nb_noise_loglike(table._h, full, None, 0, None, 0, 0, None,
                                None) == 0
    assert lib.nb_noise_destroy(None) == 0
    # shapes that do not fit together never reach the library
    with pytest.raises(ValueError):
        device.NoiseTable(d, np.ones(4))
    with pytest.raises(ValueError):
        device.NoiseTable(d.reshape(3, 1))
    with pytest.raises(ValueError):
        table.loglike(m, w3[:3], row)


@pytest.mark.parametrize('mode', MODES)
def test_from_model_layout_rules(mode):
    import torch
    d, sigma, m, w = problem(17, 1000, mode)
    like = make(d, sigma, mode, normalised=True)
    mt, wt = torch.from_numpy(m).cuda(), torch.from_numpy(w).cuda()
    for args in ((mt[:, :16], wt), (mt[0], wt), (mt.float(), wt),
                 (mt, wt.float()), (mt, wt[:, :2]), (mt, wt[:999]),
                 (mt, w), (m, wt)):
        with pytest.raises(ValueError):
            like.from_model(*args)
    want = like.from_model(mt, wt)
    # anything but unit-stride rows is copied, and gives the same bits
    turned = mt.t().contiguous().t()
    assert turned.stride() == (1, 1000)
    wturned = wt.t().contiguous().t()
    assert wturned.stride() == (1, 1000)
    assert torch.equal(like.from_model(turned, wt), want)
    assert torch.equal(like.from_model(mt, wturned), want)
    twice = torch.stack([mt, mt], dim=2)[:, :, 0]       # stride(1) == 2
    wtwice = torch.stack([wt, wt], dim=2)[:, :, 0]
    assert twice.stride(1) == 2 and wtwice.stride(1) == 2
    assert torch.equal(like.from_model(twice, wtwice), want)
    # numpy in, numpy out
    out = like.from_model(m, w)
    assert isinstance(out, np.ndarray) and out.dtype == np.float64
    assert np.array_equal(out, want.cpu().numpy())
    from nautilus_amd import GaussianNoiseLikelihood
    both = GaussianNoiseLikelihood(lambda x: (x, wt), d, sigma, noise=mode)
    called = both(m)
    assert isinstance(called, np.ndarray)
    assert np.array_equal(called, out)
    assert both(mt).is_cuda and torch.equal(both(mt), want)


def test_unit_inflation_against_the_data_vector_likelihood():
    """Row mode with w = (1, 0, 0) is ``GaussianDataLikelihood(sigma=...)``
    minus sum log sigma, both without the constant, within the sum of the two
    budgets: this file's and, for the diagonal chi^2 kernel, the one its own
    tests use (test_data_likelihood_gpu.reference and _check: 4 (P + 2) eps
    sum (r / sigma)^2 on chi^2, half of it on log L), plus one rounding for
    the subtraction."""
    import torch
    from nautilus_amd import GaussianDataLikelihood
    d, sigma, m, w = unit_inflation_problem()
    p = len(d)
    mt, wt = torch.from_numpy(m).cuda(), torch.from_numpy(w).cuda()
    got = make(d, sigma, 'row').from_model(mt, wt).cpu().numpy()
    other = GaussianDataLikelihood(identity, d, sigma=sigma, normalised=False)
    log_sigma = float(np.sum(np.log(sigma.astype(np.longdouble))))
    want = other.from_model(mt).cpu().numpy() - log_sigma
    _, x, a, _, _ = reference(d, sigma, m, w, 'row')
    tol = budget(p, x, a) + 2 * (p + 2) * EPS * x + EPS * np.abs(want)
    used = np.abs(got - want) / tol
    print('largest used fraction of the two budgets %.3g' % used.max())
    assert np.all(used <= 1.0), used.max()


# ---------------------------------------------------------- through Sampler

MU_TRUE, JITTER_SD = 0.3, 0.2
A_MAX = 0.5


@functools.lru_cache(maxsize=None)
def _jitter_problem():
    """24 measurements of a constant 0.3 with error bars between 0.05 and
    0.15 and a jitter of 0.2 added in quadrature, drawn once."""
    rng = np.random.default_rng(2026)
    sigma = 0.05 + 0.1 * rng.random(24)
    data = MU_TRUE + np.sqrt(sigma**2 + JITTER_SD**2) * rng.normal(size=24)
    return data, sigma


def _run_jitter():
    import torch
    from scipy import stats
    from nautilus_amd import GaussianNoiseLikelihood, Prior, Sampler
    data, sigma = _jitter_problem()
    prior = Prior()
    prior.add_parameter('mu', dist=stats.uniform(-1.0, 2.0))
    prior.add_parameter('a', dist=stats.uniform(0.0, A_MAX))
    assert prior.device                  # transformed on the GPU

    def model(x):
        w = torch.stack([torch.ones_like(x[:, 1]), x[:, 1],
                         torch.zeros_like(x[:, 1])], dim=1)
        return x[:, 0:1].expand(-1, 24), w

    like = GaussianNoiseLikelihood(model, data, sigma)
    s = Sampler(prior, like, pass_dict=False, n_live=1000, n_networks=2,
                vectorized=True, seed=0)
    s.run(n_eff=5000, discard_exploration=True)
    return like, s


def _quadrature():
    """log Z and the posterior means and standard deviations of (mu, a): for
    a given jitter variance a the mu-integral over (-1, 1) is a Gaussian one
    (erf at the two ends, through ``truncnorm``); the integral over a is
    ``scipy.integrate.quad``."""
    from math import erf
    from scipy import integrate
    data, sigma = _jitter_problem()

    def parts(a):
        v = sigma**2 + a
        wsum = np.sum(1 / v)
        hat = np.sum(data / v) / wsum
        rest = np.sum(data**2 / v) - wsum * hat**2
        sd = 1 / np.sqrt(wsum)
        # N(hat, sd^2) cut at -1 and 1: its mass, mean and variance
        lo, hi = (-1 - hat) / sd, (1 - hat) / sd
        mass = 0.5 * (erf(hi / np.sqrt(2)) - erf(lo / np.sqrt(2)))
        pdf = np.exp(-0.5 * np.array([lo, hi])**2) / np.sqrt(2 * np.pi)
        lean = (pdf[0] - pdf[1]) / mass
        mean = hat + sd * lean
        var = sd**2 * (1 + (lo * pdf[0] - hi * pdf[1]) / mass - lean**2)
        # density of the data integrated over mu in (-1, 1), prior 1/2
        log_g = -0.5 * np.sum(np.log(2 * np.pi * v)) - 0.5 * rest + \
            0.5 * np.log(2 * np.pi) + np.log(sd) + np.log(mass) + np.log(0.5)
        return log_g, mean, var

    shift = max(parts(a)[0] for a in np.linspace(1e-4, A_MAX, 200))

    def integral(fun):
        return integrate.quad(
            lambda a: np.exp(parts(a)[0] - shift) * fun(a, *parts(a)[1:]),
            0.0, A_MAX, epsabs=0, epsrel=1e-10, limit=200)[0] / A_MAX

    z = integral(lambda a, mean, var: 1.0)
    mu1 = integral(lambda a, mean, var: mean) / z
    mu2 = integral(lambda a, mean, var: var + mean**2) / z
    a1 = integral(lambda a, mean, var: a) / z
    a2 = integral(lambda a, mean, var: a * a) / z
    return np.log(z) + shift, np.array([mu1, a1]), \
        np.sqrt(np.array([mu2 - mu1**2, a2 - a1**2]))


def test_sampler_recovers_mean_and_jitter():
    """Evidence and posterior means in the settings and the evidence band of
    test_sampler_recovers_rates (test_poisson_likelihood_gpu.py), against
    quadrature."""
    log_z, mean, sd = _quadrature()
    like, s = _run_jitter()
    print('log Z = %.4f, quadrature %.4f, n_like = %d, n_eff = %.0f' % (
        s.log_z, log_z, s.n_like, s.n_eff))
    assert abs(s.log_z - log_z) < 0.06
    pts, log_w, _ = s.posterior()
    wgt = np.exp(log_w - np.max(log_w))
    got = wgt @ pts / wgt.sum()
    tol = 4 * sd / np.sqrt(s.n_eff)
    print('posterior mean - quadrature mean in units of the tolerance:',
          (got - mean) / tol, 'means', mean, 'sd', sd)
    assert np.all(np.abs(got - mean) < tol)
    _, again = _run_jitter()
    assert again.log_z == s.log_z and again.n_like == s.n_like
