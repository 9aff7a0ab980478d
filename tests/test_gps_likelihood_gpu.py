"""The device Gaussian-process likelihood of an ordered series
(``nb_gps_loglike``, nautilus_amd/csrc/nb_gps_filter.h) against its recursion
in ``np.longdouble``, its bit-for-bit independence of the batch, its NaN rules,
the dense kernel ``nb_gp_loglike`` on the same inputs, a series of 2^20
samples, and end to end through ``Sampler``.  The problems, the truth and the
tolerance (``case_budget``: eight times the float64 twin's own error against
the truth, at least 64 eps of the value) live in test_gps_likelihood.py."""

import functools

import numpy as np
import pytest

import test_gp_likelihood as dense
from test_gps_likelihood import (BAD_HYPER, BAD_Q, DENSE_N, EPS, LD, SHARED,
                                 budget, case_budget, identity, make, problem,
                                 truth)

pytestmark = pytest.mark.gpu

KERNELS = ('exp', 'matern32', 'matern52', 'sho')
N_ALL = (1, 63, 64, 65, 130)


def block():
    from nautilus_amd import device
    return device.GPS_BLOCK


def _cuda(*arrays):
    import torch
    return [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in arrays]


# index of P in (1, 2, C - 1, C, C + 1, 2 C + 1, 4096); n rotates so that every
# kernel meets every n
SHAPES = [(ip, N_ALL[(ip + ik) % 5], kernel)
          for ik, kernel in enumerate(KERNELS) for ip in range(7)]


def test_shapes():
    from nautilus_amd import device
    from nautilus_amd.likelihoods import GPS_KERNELS, N_GPS_MAX
    assert device.GPS_BLOCK >= 4 and device.GPS_BLOCK % 2 == 0
    assert tuple(device.GPS_KERNELS) == GPS_KERNELS == KERNELS
    assert [device.GPS_KERNELS[k] for k in KERNELS] == [0, 1, 2, 3]
    assert device.GPS_MAX_DATA == N_GPS_MAX
    assert device.GPS is device.GPSTable
    for kernel in KERNELS:
        assert {n for _, n, k in SHAPES if k == kernel} == set(N_ALL)


@pytest.mark.parametrize('ip, n, kernel', SHAPES)
def test_values(ip, n, kernel):
    """|device - long double| <= case_budget in every row."""
    import torch
    c = block()
    p = (1, 2, c - 1, c, c + 1, 2 * c + 1, 4096)[ip]
    t, d, sigma, m, h = problem(p, n, kernel)
    want = truth(p, n, kernel)
    tol = case_budget(p, n, kernel)
    raw = make(t, d, sigma, kernel)
    mt, ht = _cuda(m, h)
    out = raw.from_model(mt, ht)
    assert out.is_cuda and out.dtype == torch.float64 and out.shape == (n,)
    got = out.cpu().numpy()
    err = np.abs(got.astype(LD) - want).astype(float)
    print('P = %d, n = %d, %s: largest used fraction of the tolerance %.3g '
          '(largest error %.3g, relative %.3g)' % (
              p, n, kernel, (err / tol).max(), err.max(),
              (err / np.abs(want.astype(float))).max()))
    assert np.all(np.isfinite(got))
    assert np.all(err <= tol), (err / tol).max()
    # the constant joins with one subtraction: log_norm - sum / 2
    like = make(t, d, sigma, kernel, normalised=True)
    assert like.log_norm == -0.5 * p * np.log(2 * np.pi)
    assert np.array_equal(like.from_model(mt, ht).cpu().numpy(),
                          like.log_norm + got)
    # numpy in, numpy out
    if ip == 4:
        assert np.array_equal(raw.from_model(m, h), got)


@pytest.mark.parametrize('kernel', KERNELS)
def test_rows_bit_for_bit(kernel):
    """A row's bits are those it has alone, inside a batch of 17 and inside a
    batch of 130 at different positions, with m and h each in place inside a
    wider tensor, on any stream."""
    import torch
    n, p = 130, 2 * block() + 6
    width = 4 if kernel == 'sho' else 3
    t, d, sigma, m, h = problem(p, n, kernel)
    like = make(t, d, sigma, kernel, normalised=True)
    big, hbig = _cuda(m, h)
    full = like.from_model(big, hbig)
    assert bool(torch.isfinite(full).all())
    for off in (0, 1, 60, 113):
        sub, hsub = big[off:off + 17], hbig[off:off + 17]
        assert sub.data_ptr() == big.data_ptr() + off * p * 8   # a view
        assert torch.equal(like.from_model(sub, hsub), full[off:off + 17]), off
        for r in (off, off + 16):
            assert torch.equal(like.from_model(big[r:r + 1], hbig[r:r + 1]),
                               full[r:r + 1])
    perm = torch.from_numpy(np.random.default_rng(p).permutation(n)).cuda()
    assert torch.equal(like.from_model(big[perm], hbig[perm]), full[perm])
    assert like.from_model(big[:0], hbig[:0]).shape == (0,)
    # slices of wider tensors, m and h independently; odd strides both
    rng = np.random.default_rng(p)
    wide = torch.from_numpy(rng.normal(size=(n, p + 5))).cuda()
    wide[:, 3:3 + p] = big
    view = wide[:, 3:3 + p]
    assert view.data_ptr() == wide.data_ptr() + 3 * 8
    assert view.stride() == (p + 5, 1)
    hwide = torch.from_numpy(rng.normal(size=(n, 7))).cuda()
    hwide[:, 1:1 + width] = hbig
    hview = hwide[:, 1:1 + width]
    assert hview.data_ptr() == hwide.data_ptr() + 8
    assert hview.stride() == (7, 1)
    assert torch.equal(like.from_model(view, hbig), full)
    assert torch.equal(like.from_model(big, hview), full)
    assert torch.equal(like.from_model(view, hview), full)
    table = like._table()
    assert torch.equal(table.loglike(view, hview, ld=p + 5, ld_hyper=7), full)
    assert torch.equal(table.loglike(view[5:22], hview[5:22]), full[5:22])
    # columns that are not contiguous are copied, not misread
    assert torch.equal(like.from_model(big.t().contiguous().t(), hbig), full)
    # a stream of its own
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        other = like.from_model(big, hbig)
        one = like.from_model(view[9:10], hview[9:10])
    stream.synchronize()
    assert torch.equal(other, full) and torch.equal(one, full[9:10])


@pytest.mark.parametrize('kernel', KERNELS)
def test_edge_rows(kernel):
    """Every cause of a NaN row in the first, a middle and the last lane of a
    wavefront and in the tail wavefront; the other rows keep their bits."""
    import torch
    n, p = 130, block() + 3
    t, d, sigma, m, h = problem(p, n, kernel)
    like = make(t, d, sigma, kernel)
    mt, ht = _cuda(m, h)
    clean = like.from_model(mt, ht)
    assert bool(torch.isfinite(clean).all())
    places = [0, 31, 63, 64, 127, 129]
    rest = torch.ones(n, dtype=torch.bool, device='cuda')
    rest[places] = False
    causes = [('h', col, v) for col, v in
              BAD_HYPER + (BAD_Q if kernel == 'sho' else [])]
    causes += [('m', col, v) for col in (0, block() - 1, block(), p - 1)
               for v in (float('nan'), float('inf'), -float('inf'))]
    for what, col, value in causes:
        m2, h2 = mt.clone(), ht.clone()
        (h2 if what == 'h' else m2)[places, col] = value
        got = like.from_model(m2, h2)
        assert bool(torch.isnan(got[places]).all()), (what, col, value)
        assert torch.equal(got[rest], clean[rest]), (what, col, value)
    # all causes at once, one per place
    m2, h2 = mt.clone(), ht.clone()
    for i, (what, col, value) in zip(places, causes[::3]):
        (h2 if what == 'h' else m2)[i, col] = value
    got = like.from_model(m2, h2)
    assert bool(torch.isnan(got[places]).all())
    assert torch.equal(got[rest], clean[rest])
    # a = 0 is white noise.  Equal times (problem has a pair) are finite with
    # noise, as above; without any (sigma = s = 0, a > 0) the second of the
    # pair has a zero pivot: a NaN row and nothing worse
    h3 = ht.clone()
    h3[:, 0] = 0.0
    assert bool(torch.isfinite(like.from_model(mt, h3)).all())
    bare = make(t, d, None, kernel)
    h4 = ht.clone()
    h4[places, 2] = 0.0
    got = bare.from_model(mt, h4)
    assert bool(torch.isnan(got[places]).all())
    assert bool(torch.isfinite(got[rest]).all())
    assert torch.equal(got[rest], bare.from_model(mt, ht)[rest])


@pytest.mark.parametrize('kernel', SHARED)
@pytest.mark.parametrize('p', (16, 128))
def test_against_the_dense_kernel(p, kernel):
    """``nb_gps_loglike`` against ``nb_gp_loglike`` on the same inputs, within
    the sum of the two budgets."""
    from nautilus_amd import GaussianProcessLikelihood
    t, d, sigma, m, h = problem(p, DENSE_N, kernel)
    mt, ht = _cuda(m, h)
    got = make(t, d, sigma, kernel).from_model(mt, ht).cpu().numpy()
    other = GaussianProcessLikelihood(identity, t, d, sigma, kernel=kernel,
                                      cov='hyper', normalised=False)
    want = other.from_model(mt, ht).cpu().numpy()
    ref = dense.reference(other.dist, d, sigma, m, h, 'hyper', kernel)
    tol = case_budget(p, DENSE_N, kernel) + \
        dense.budget(p, ref, h[:, 0]).total
    err = np.abs(got - want)
    print('P = %d, %s: largest used fraction of the two budgets %.3g' % (
        p, kernel, (err / tol).max()))
    assert np.all(np.isfinite(got)) and np.all(np.isfinite(want))
    assert np.all(err <= tol), (err / tol).max()


def test_long_series():
    """P = 2^20 (the index arithmetic at the limit), white noise, against the
    closed form; tolerance 8 eps sum_j |term_j| per row."""
    import torch
    p, n = 1 << 20, 64
    rng = np.random.default_rng(20)
    t = np.cumsum(rng.uniform(0, 2e-5, size=p))
    t[1000] = t[999]
    sigma = rng.uniform(0.1, 1, size=p)
    d = rng.normal(size=p)
    m = rng.standard_normal(size=(n, p))
    m *= 0.5
    m += d
    h = np.stack([np.zeros(n), 10.0**rng.uniform(-1.5, 1, size=n),
                  10.0**rng.uniform(-4, -1, size=n)], axis=1)
    like = make(t, d, sigma, 'matern32')
    mt, ht = _cuda(m, h)
    got = like.from_model(mt, ht).cpu().numpy()
    del mt
    want, total = np.empty(n), np.empty(n)
    for i in range(n):
        v = sigma * sigma + h[i, 2]
        chi, log_v = (m[i] - d)**2 / v, np.log(v)
        want[i] = -0.5 * (np.sum(chi) + np.sum(log_v))
        total[i] = 0.5 * (np.sum(chi) + np.sum(np.abs(log_v)))
    err = np.abs(got - want)
    print('P = 2^20: largest used fraction of the tolerance %.3g' %
          (err / (8 * EPS * total)).max())
    assert np.all(np.isfinite(got))
    assert np.all(err <= 8 * EPS * total)


def test_long_correlated_series():
    """P = 8192, Matern-3/2, against the twin under ``case_budget``."""
    p, n = 8192, 64
    t, d, sigma, m, h = problem(p, n, 'matern32')
    got = make(t, d, sigma, 'matern32').from_model(*_cuda(m, h)).cpu().numpy()
    err = np.abs(got.astype(LD) - truth(p, n, 'matern32')).astype(float)
    tol = case_budget(p, n, 'matern32')
    print('P = 8192: largest used fraction of the tolerance %.3g' %
          (err / tol).max())
    assert np.all(np.isfinite(got))
    assert np.all(err <= tol), (err / tol).max()


def test_one_handle_on_two_streams():
    import torch
    from nautilus_amd import GaussianProcessSeriesLikelihood
    t, d, sigma, m, h = problem(65, 130, 'sho')
    ht, x = _cuda(h, m)
    like = GaussianProcessSeriesLikelihood(lambda x: (x, ht), t, d, sigma,
                                           kernel='sho')
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
    # numpy points in, numpy out
    assert np.array_equal(like(m), want.cpu().numpy())


def test_argument_errors_carry_err_arg():
    import ctypes
    import torch
    from nautilus_amd import _lib, device

    def code(*args, **kw):
        with pytest.raises(_lib.NativeError) as err:
            device.GPSTable(*args, **kw)
        assert str(err.value) != 'nautilus_hip: '
        return err.value.code

    t = np.array([0.0, 1.0, 1.0])
    d = np.array([0.5, -2.0, 5.5])
    assert device.GPSTable(t, d).n_data == 3
    assert device.GPSTable(t, d, np.r_[0.0, 1.0, 4.0], kernel='sho',
                           log_norm=-3.0).width == 4
    assert code(np.zeros(0), np.zeros(0)) == _lib.ERR_ARG
    assert code(np.zeros((1 << 20) + 1), np.zeros((1 << 20) + 1)) == \
        _lib.ERR_ARG
    assert code(t, np.r_[1.0, np.nan, 1.0]) == _lib.ERR_ARG
    for bad in (np.r_[0.0, 2.0, 1.0], np.r_[0.0, np.nan, 1.0],
                np.r_[0.0, 1.0, np.inf], np.r_[-1.5e308, 1.5e308, 1.5e308]):
        assert code(bad, d) == _lib.ERR_ARG
    for bad in (-1e-300, np.nan, np.inf):
        assert code(t, d, np.r_[0.0, bad, 1.0]) == _lib.ERR_ARG
    assert code(t, d, log_norm=np.nan) == _lib.ERR_ARG
    lib = _lib.load()
    h = ctypes.c_void_p()

    def raw_refused(fn, *args):
        # another entry's message first: the text checked below is this call's
        assert lib.nb_poisson_create(0, None, None, None, 0.0,
                                     None) == _lib.ERR_ARG
        assert b'Poisson' in lib.nb_last_error()
        assert fn(*args) == _lib.ERR_ARG
        assert b'Gaussian-process series likelihood' in lib.nb_last_error()

    tp = t.ctypes.data_as(_lib.c_double_p)
    dp = d.ctypes.data_as(_lib.c_double_p)
    raw_refused(lib.nb_gps_create, 3, None, dp, None, 0, 0.0, ctypes.byref(h))
    raw_refused(lib.nb_gps_create, 3, tp, None, None, 0, 0.0, ctypes.byref(h))
    raw_refused(lib.nb_gps_create, 3, tp, dp, None, 0, 0.0, None)
    raw_refused(lib.nb_gps_create, 3, tp, dp, None, 4, 0.0, ctypes.byref(h))
    raw_refused(lib.nb_gps_create, 3, tp, dp, None, -1, 0.0, ctypes.byref(h))
    table = device.GPSTable(t, d, np.ones(3))
    sho = device.GPSTable(t, d, np.ones(3), kernel='sho')
    m = torch.ones(4, 3, dtype=torch.float64, device='cuda')
    h3 = torch.ones(4, 3, dtype=torch.float64, device='cuda')
    h4 = torch.ones(4, 4, dtype=torch.float64, device='cuda')

    def refused(tab, *args, **kw):
        with pytest.raises(_lib.NativeError) as err:
            tab.loglike(*args, **kw)
        assert err.value.code == _lib.ERR_ARG
        assert 'Gaussian-process series likelihood' in str(err.value)
        return str(err.value)

    # ld and ld_hyper count from the second row on
    assert 'ld_hyper >= 3' in refused(table, m, h3, ld=2)
    refused(table, m, h3, ld_hyper=2)
    assert 'ld_hyper >= 4' in refused(sho, m, h4, ld_hyper=3)
    refused(sho, m, h4, ld=2)
    want = table.loglike(m, h3)
    assert want.shape == (4,) and bool(torch.isfinite(want).all())
    assert torch.equal(table.loglike(m, h3, ld=3, ld_hyper=3), want)
    assert torch.equal(table.loglike(m[:1], h3[:1], ld=0, ld_hyper=0),
                       want[:1])
    assert torch.equal(sho.loglike(m[:1], h4[:1], ld=0, ld_hyper=0),
                       sho.loglike(m, h4)[:1])
    # NULL pointers with n > 0, and none needed for n = 0
    out = torch.empty(4, dtype=torch.float64, device='cuda')
    ptrs = dict(h=table._h, m=m.data_ptr(), c=h3.data_ptr(),
                out=out.data_ptr())
    for null in ('h', 'm', 'c', 'out'):
        a = dict(ptrs)
        a[null] = None
        raw_refused(lib.nb_gps_loglike, a['h'], a['m'], 3, a['c'], 3, 4,
                    a['out'], None)
    raw_refused(lib.nb_gps_loglike, table._h, m.data_ptr(), 3, h3.data_ptr(),
                3, -1, out.data_ptr(), None)
    assert lib.nb_gps_loglike(table._h, None, 3, None, 3, 0, None, None) == 0
    assert lib.nb_gps_loglike(sho._h, None, 0, None, 0, 0, None, None) == 0
    assert lib.nb_gps_destroy(None) == 0
    # shapes that do not fit together never reach the library
    with pytest.raises(ValueError):
        device.GPSTable(t, d, np.ones(4))
    with pytest.raises(ValueError):
        device.GPSTable(t[:2], d)
    with pytest.raises(ValueError):
        device.GPSTable(t, d, kernel='sqexp')
    with pytest.raises(ValueError):
        table.loglike(m, h3[:3])


# ---------------------------------------------------------- through Sampler

SERIES_TRUE = (0.7, 1.0, 1.5, 0.01)           # mean, a, l, s
SERIES_SIGMA = 0.05
SERIES_P = 1024


@functools.lru_cache(maxsize=None)
def _series():
    """1024 samples of a Matern-3/2 process with a constant mean at sorted
    uniform times in [0, 300], error bars of 0.05, drawn once."""
    from nautilus_amd.likelihoods import gp_correlation
    rng = np.random.default_rng(2028)
    t = np.sort(rng.uniform(0, 300, size=SERIES_P))
    mean, a, l, s = SERIES_TRUE
    k = a * gp_correlation('matern32', np.abs(t[:, None] - t[None, :]) / l) + \
        (s + SERIES_SIGMA**2) * np.eye(SERIES_P)
    return t, mean + np.linalg.cholesky(k) @ rng.normal(size=SERIES_P)


def test_sampler_recovers_the_hyper_parameters():
    """Mean, log a, log l and log s of a simulated series through ``Sampler``
    with a device prior: every truth within four posterior standard
    deviations of the posterior mean, and the run repeats bit for bit."""
    from scipy import stats
    from nautilus_amd import GaussianProcessSeriesLikelihood, Prior, Sampler
    t, data = _series()

    def model(x):
        return x[:, :1].expand(x.shape[0], SERIES_P), x[:, 1:]

    def run():
        like = GaussianProcessSeriesLikelihood(
            model, t, data, np.full(SERIES_P, SERIES_SIGMA),
            kernel='matern32')
        prior = Prior()
        prior.add_parameter('mean', dist=stats.uniform(-3.0, 6.0))
        for name, (lo, hi) in zip('als', ((0.05, 20.0), (0.1, 20.0),
                                          (1e-4, 1.0))):
            prior.add_parameter(name, dist=stats.loguniform(lo, hi))
        assert prior.device                  # transformed on the GPU
        s = Sampler(prior, like, pass_dict=False, n_live=400,
                    vectorized=True, seed=0)
        s.run(n_eff=2000, discard_exploration=True)
        return s

    s = run()
    pts, log_w, _ = s.posterior()
    wgt = np.exp(log_w - np.max(log_w))
    x = np.concatenate([pts[:, :1], np.log(pts[:, 1:])], axis=1)
    mean = wgt @ x / wgt.sum()
    sd = np.sqrt(wgt @ (x - mean)**2 / wgt.sum())
    want = np.r_[SERIES_TRUE[0], np.log(SERIES_TRUE[1:])]
    print('log Z = %.3f, n_like = %d, n_eff = %.0f; (mean - truth) / sd:' % (
        s.log_z, s.n_like, s.n_eff), (mean - want) / sd, 'sd', sd)
    assert np.all(np.isfinite(mean)) and np.all(sd > 0)
    assert np.all(np.abs(mean - want) < 4 * sd)
    again = run()
    assert again.log_z == s.log_z and again.n_like == s.n_like
