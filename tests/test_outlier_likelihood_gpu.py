"""The fused device Gaussian likelihood with outliers (``nb_outlier_loglike``,
nautilus_amd/csrc/nb_outlier.hip) against the defining formula in
``np.longdouble`` under a derived error bound, its bit-for-bit independence of
the batch, its NaN rules, and end to end through ``Sampler``.  The problems,
the reference and the bound (``budget``, with its derivation) live in
test_outlier_likelihood.py, which holds the numpy twin to them without a
GPU."""

import functools

import numpy as np
import pytest

from test_noise_likelihood import budget as noise_budget
from test_noise_likelihood import reference as noise_reference
from test_outlier_likelihood import (EDGE_TEST_P, LONG_SHAPE, ROW_TEST_P,
                                     SHAPES, budget, check_classes, expected,
                                     identity, long_expected, long_problem,
                                     make, problem, reference)

pytestmark = pytest.mark.gpu


def test_shapes_cover_both_sides_of_every_launcher_boundary():
    from nautilus_amd import device
    ps = sorted({s[0] for s in SHAPES})
    shapes = [device.outlier_launch_shape(p) for p in range(1, 5001)]
    changes = [p for p in range(1, 5000) if shapes[p - 1] != shapes[p]]
    assert changes
    for p in changes:
        assert p in ps and p + 1 in ps
    for p in (1, 3, 15, 16, 17, 63, 64, 65, 4099):
        assert p in ps
    # the bit-for-bit and the edge tests run on every shape
    for group in (ROW_TEST_P, EDGE_TEST_P):
        assert {device.outlier_launch_shape(p) for p in group} == set(shapes)


@pytest.mark.parametrize('p, n, rot', SHAPES)
def test_values(p, n, rot):
    """|device - long double| <= budget(P, X, A, Y) and finite in every row
    (the budget is derived in test_outlier_likelihood.budget)."""
    import torch
    check_classes(p, n, rot)
    d, sigma, m, w = problem(p, n, rot)
    want, x, a, y, _ = expected(p, n, rot)
    tol = budget(p, x, a, y)
    raw = make(d, sigma)
    mt, wt = torch.from_numpy(m).cuda(), torch.from_numpy(w).cuda()
    out = raw.from_model(mt, wt)
    assert out.is_cuda and out.dtype == torch.float64 and out.shape == (n,)
    got = out.cpu().numpy()
    used = np.abs(got - want) / tol
    print('P = %d, n = %d, rot = %d: largest used fraction of the bound '
          '%.3g' % (p, n, rot, used.max()))
    assert np.all(np.isfinite(got))
    assert np.all(np.abs(got - want) <= tol), used.max()
    # the constant joins with one addition: log_norm + sum
    like = make(d, sigma, normalised=True)
    assert like.log_norm == -0.5 * p * np.log(2 * np.pi)
    assert np.array_equal(like.from_model(mt, wt).cpu().numpy(),
                          like.log_norm + got)


def test_long_row():
    """Every B in [1, 1.001): each mantissa is about 1/2, and a lane's
    running product is renormalised twice on its way."""
    import torch
    p, n = LONG_SHAPE
    d, sigma, m, w = long_problem(p, n)
    want, x, a, y, kinds = long_expected()
    assert 1.0 <= kinds['b_min'] and kinds['b_max'] < 1.001
    tol = budget(p, x, a, y)
    out = make(d, sigma).from_model(torch.from_numpy(m).cuda(),
                                    torch.from_numpy(w).cuda())
    got = out.cpu().numpy()
    used = np.abs(got - want) / tol
    print('P = %d, n = %d: largest used fraction of the bound %.3g' % (
        p, n, used.max()))
    assert np.all(np.isfinite(got))
    assert np.all(np.abs(got - want) <= tol), used.max()


def test_no_outliers_against_the_noise_kernel():
    """The p = 0 rows against ``nb_noise_loglike`` in row mode on the same
    tensors (its (c, a, f) are the first three columns of the mixture, read in
    place), within the sum of the two budgets."""
    import torch
    from nautilus_amd import device
    p, n = 65, 1000
    d, sigma, m, w = problem(p, n)
    rows = np.flatnonzero(w[:, 3] == 0.0)
    assert len(rows) == 200
    m, w = np.ascontiguousarray(m[rows]), np.ascontiguousarray(w[rows])
    mt, wt = torch.from_numpy(m).cuda(), torch.from_numpy(w).cuda()
    table = make(d, sigma)._table()
    got = table.outlier_loglike(mt, wt).cpu().numpy()
    cut = wt[:, :3]
    assert cut.data_ptr() == wt.data_ptr() and cut.stride() == (6, 1)
    want = table.loglike(mt, cut, device.NOISE_ROW).cpu().numpy()
    _, x, a, y, kinds = reference(d, sigma, m, w)
    assert kinds['p0_outlier_larger'] > 0 and np.all(y == 0.0)
    _, nx, na, _, _ = noise_reference(d, sigma, m, w[:, :3], 'row')
    tol = budget(p, x, a, y) + noise_budget(p, nx, na)
    assert np.all(np.isfinite(want)) and np.all(np.isfinite(got))
    used = np.abs(got - want) / tol
    print('largest used fraction of the two budgets %.3g' % used.max())
    assert np.all(used <= 1.0), used.max()


@pytest.mark.parametrize('p', ROW_TEST_P)
def test_rows_bit_for_bit(p):
    """A row's bits are those it has alone, inside batches of 17 and 4097 at
    different positions, with m and w each in place inside a wider tensor, on
    any stream."""
    import torch
    d, sigma, m, w = problem(p, 4097)
    like = make(d, sigma, normalised=True)
    width = 6
    big, mix = torch.from_numpy(m).cuda(), torch.from_numpy(w).cuda()
    full = like.from_model(big, mix)
    assert bool(torch.isfinite(full).all())
    for off in (0, 1, 777, 4080):
        sub, wsub = big[off:off + 17], mix[off:off + 17]
        assert sub.data_ptr() == big.data_ptr() + off * p * 8   # a view
        assert wsub.data_ptr() == mix.data_ptr() + off * width * 8
        assert torch.equal(like.from_model(sub, wsub), full[off:off + 17]), off
        for r in (off, off + 16):
            assert torch.equal(like.from_model(big[r:r + 1], mix[r:r + 1]),
                               full[r:r + 1])
    # the same rows at other positions of a batch
    perm = torch.from_numpy(np.random.default_rng(p).permutation(4097)).cuda()
    assert torch.equal(like.from_model(big[perm], mix[perm]), full[perm])
    assert like.from_model(big[:0], mix[:0]).shape == (0,)
    # column slices of wider tensors, m and w independently
    rng = np.random.default_rng(p)
    wide = torch.from_numpy(rng.normal(size=(4097, p + 5))).cuda()
    wide[:, 2:2 + p] = big
    view = wide[:, 2:2 + p]
    assert view.data_ptr() == wide.data_ptr() + 2 * 8
    assert view.stride() == (p + 5, 1)
    wwide = torch.from_numpy(rng.normal(size=(4097, width + 3))).cuda()
    wwide[:, 1:1 + width] = mix
    wview = wwide[:, 1:1 + width]
    assert wview.data_ptr() == wwide.data_ptr() + 8
    assert wview.stride() == (width + 3, 1)
    assert torch.equal(like.from_model(view, mix), full)
    assert torch.equal(like.from_model(big, wview), full)
    assert torch.equal(like.from_model(view, wview), full)
    table = like._table()
    assert torch.equal(table.outlier_loglike(view, wview, ld=p + 5,
                                             ld_mix=width + 3), full)
    assert torch.equal(table.outlier_loglike(view[5:22], wview[5:22]),
                       full[5:22])
    assert torch.equal(table.outlier_loglike(view[40:41], mix[40:41]),
                       full[40:41])
    # a stream of its own
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        other = like.from_model(big, mix)
        one = like.from_model(view[9:10], wview[9:10])
    stream.synchronize()
    assert torch.equal(other, full) and torch.equal(one, full[9:10])


@pytest.mark.parametrize('p', EDGE_TEST_P)
def test_edge_rows(p):
    """Every NaN rule planted in single rows of a 100-row batch: the other
    rows keep their bits, and the NaN pattern is the twin's."""
    import torch
    d, sigma, m, w = problem(p, 1000)
    like = make(d, sigma, normalised=True)
    cm = torch.from_numpy(m[:100].copy()).cuda()
    cw = torch.from_numpy(w[:100].copy()).cuda()
    want = like.from_model(cm, cw)
    assert bool(torch.isfinite(want).all())
    cls = np.arange(p) % 4
    c_zero = int(np.flatnonzero(cls == 0)[-1])          # sigma_j = 0
    c_last = p - 1
    assert sigma[c_zero] == 0
    nan, inf = float('nan'), float('inf')
    dm, dw = cm.clone(), cw.clone()
    plant = {
        # m not finite
        40: (dm, 0, nan), 41: (dm, c_last, inf), 42: (dm, 1, -inf),
        # v outside (0, +inf): zero at sigma_j = 0, negative, infinite, NaN
        3: (dw, slice(0, 3), (1.0, 0.0, 0.0)),
        11: (dw, slice(0, 3), (1.0, -1e13, 0.0)),
        12: (dw, 1, inf), 13: (dw, 0, nan), 14: (dw, 2, nan),
        77: (dw, slice(0, 3), (0.0, 0.0, 0.0)), 99: (dw, 1, -inf),
        # u outside (0, +inf): zero at sigma_j = 0, negative, infinite, NaN
        20: (dw, 5, 0.0), 21: (dw, 5, -1e13), 22: (dw, 5, inf),
        23: (dw, 5, nan), 24: (dw, 5, -inf),
        # p outside [0, 1]
        30: (dw, 3, -1e-300), 31: (dw, 3, 1.0 + 2.0**-52), 32: (dw, 3, nan),
        33: (dw, 3, inf), 34: (dw, 3, -inf), 35: (dw, 3, 2.0),
        # b not finite, also where p = 0 (row 50)
        50: (dw, 4, nan), 51: (dw, 4, inf), 52: (dw, 4, -inf),
        53: (dw, 4, nan),
    }
    assert float(cw[50, 3]) == 0.0
    for i, (t, col, value) in plant.items():
        t[i, col] = torch.tensor(value, dtype=torch.float64, device='cuda')
    bad = sorted(plant)
    out = like.from_model(dm, dw)
    for i in bad:
        assert bool(torch.isnan(out[i])), i
    keep = torch.ones(100, dtype=torch.bool, device='cuda')
    keep[bad] = False
    assert int(keep.sum()) == 100 - len(bad)
    assert torch.equal(out[keep], want[keep])
    twin = like.numpy_from_model(dm.cpu().numpy(), dw.cpu().numpy())
    assert np.array_equal(np.isnan(twin), torch.isnan(out).cpu().numpy())
    # the sign of a single coefficient does not matter while v > 0
    sm, sw = cm[5:6].clone(), cw[5:6].clone()
    sw[0, :3] = torch.tensor([-1e-13, float(sigma.max()**2) + 1.0, 0.5])
    got = like.from_model(sm, sw)
    assert bool(torch.isfinite(got).all())
    assert np.isfinite(like.numpy_from_model(sm.cpu().numpy(),
                                             sw.cpu().numpy())[0])
    # p = 0 and p = 1 are legal however far the absent component lies
    zm, zw = cm[6:8].clone(), cw[6:8].clone()
    zw[0, 3], zw[1, 3] = 0.0, 1.0
    zw[0, 4] = 1e100                                    # (d - b)^2 = 1e200
    zm[1] = zm[1] + 1e100
    zw[1, 2] = 0.0                                      # v does not follow m
    got = like.from_model(zm, zw).cpu().numpy()
    ref, x, a, y, _ = reference(d, sigma, zm.cpu().numpy(), zw.cpu().numpy())
    assert np.all(np.isfinite(got))
    assert np.all(np.abs(got - (like.log_norm + ref)) <=
                  budget(p, x, a, y) + 2.0**-52 * np.abs(ref))


def test_one_handle_serves_both_kernels_on_two_streams():
    import torch
    from nautilus_amd import GaussianOutlierLikelihood, device
    d, sigma, m, w = problem(129, 1000)
    wt = torch.from_numpy(w).cuda()
    like = GaussianOutlierLikelihood(lambda x: (x, wt), d, sigma)
    x = torch.from_numpy(m).cuda()
    want = like(x)
    noise = like._table().loglike(x, wt[:, :3], device.NOISE_ROW)
    torch.cuda.synchronize()
    outs = []
    for s in (torch.cuda.Stream(), torch.cuda.Stream()):
        with torch.cuda.stream(s):
            outs.append(like(x))
            outs.append(like._table().loglike(x, wt[:, :3], device.NOISE_ROW))
    torch.cuda.synchronize()
    assert isinstance(like._table(), device.NoiseTable)
    assert like._tables and len(like._tables) == 1
    assert list(like._tables) == [torch.cuda.current_device()]
    assert torch.equal(outs[0], want) and torch.equal(outs[2], want)
    assert torch.equal(outs[1], noise) and torch.equal(outs[3], noise)


def test_argument_errors_carry_err_arg():
    import torch
    from nautilus_amd import _lib, device
    lib = _lib.load()
    d = np.array([0.5, -2.0, 5.5])
    table = device.NoiseTable(d, np.ones(3))
    m = torch.ones(4, 3, dtype=torch.float64, device='cuda')
    w6 = torch.ones(4, 6, dtype=torch.float64, device='cuda')
    w6[:, 3] = 0.25

    def raw_refused(*args):
        # another entry's message first: the text checked below is this call's
        assert lib.nb_poisson_create(0, None, None, None, 0.0,
                                     None) == _lib.ERR_ARG
        assert b'Poisson' in lib.nb_last_error()
        assert lib.nb_outlier_loglike(*args) == _lib.ERR_ARG
        assert b'outlier likelihood' in lib.nb_last_error()

    def refused(*args, **kw):
        with pytest.raises(_lib.NativeError) as err:
            table.outlier_loglike(*args, **kw)
        assert err.value.code == _lib.ERR_ARG
        assert 'outlier likelihood' in str(err.value)

    # ld and ld_mix count from the second row on
    refused(m, w6, ld=2)
    refused(m, w6, ld_mix=5)
    refused(m, w6, ld=0, ld_mix=0)
    want = table.outlier_loglike(m, w6)
    assert want.shape == (4,) and bool(torch.isfinite(want).all())
    assert torch.equal(table.outlier_loglike(m, w6, ld=3, ld_mix=6), want)
    assert torch.equal(table.outlier_loglike(m[:1], w6[:1], ld=0, ld_mix=0),
                       want[:1])
    # P = 1 still needs six doubles of mixture per row
    one = device.NoiseTable(np.zeros(1), np.ones(1))
    m1 = torch.ones(4, 1, dtype=torch.float64, device='cuda')
    with pytest.raises(_lib.NativeError):
        one.outlier_loglike(m1, w6, ld_mix=1)
    assert one.outlier_loglike(m1, w6).shape == (4,)
    # NULL pointers with n > 0, a negative n, and none needed for n = 0
    out = torch.empty(4, dtype=torch.float64, device='cuda')
    ptrs = dict(h=table._h, m=m.data_ptr(), w=w6.data_ptr(),
                out=out.data_ptr())
    for null in ('h', 'm', 'w', 'out'):
        a = dict(ptrs)
        a[null] = None
        raw_refused(a['h'], a['m'], 3, a['w'], 6, 4, a['out'], None)
    raw_refused(table._h, m.data_ptr(), 3, w6.data_ptr(), 6, -1,
                out.data_ptr(), None)
    raw_refused(table._h, m.data_ptr(), 2, w6.data_ptr(), 6, 2,
                out.data_ptr(), None)
    raw_refused(table._h, m.data_ptr(), 3, w6.data_ptr(), 5, 2,
                out.data_ptr(), None)
    assert lib.nb_outlier_loglike(table._h, None, 3, None, 6, 0, None,
                                  None) == 0
    assert lib.nb_outlier_loglike(table._h, None, 0, None, 0, 0, None,
                                  None) == 0
    assert table.outlier_loglike(m[:0], w6[:0]).shape == (0,)
    # rows that do not fit together never reach the library
    with pytest.raises(ValueError):
        table.outlier_loglike(m, w6[:3])


def test_from_model_layout_rules():
    import torch
    from nautilus_amd import GaussianOutlierLikelihood
    d, sigma, m, w = problem(17, 1000)
    like = make(d, sigma, normalised=True)
    mt, wt = torch.from_numpy(m).cuda(), torch.from_numpy(w).cuda()
    wide = torch.cat([wt, wt[:, :1]], dim=1)
    for args in ((mt[:, :16], wt), (mt[0], wt), (mt.float(), wt),
                 (mt, wt.float()), (mt, wt[:, :5]), (mt, wide),
                 (mt, wt[:999]), (mt, w), (m, wt)):
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
    both = GaussianOutlierLikelihood(lambda x: (x, wt), d, sigma)
    called = both(m)
    assert isinstance(called, np.ndarray)
    assert np.array_equal(called, out)
    assert both(mt).is_cuda and torch.equal(both(mt), want)


# ---------------------------------------------------------- through Sampler

MU_TRUE = 0.3
P_MAX = 0.5
B_OUT, S_OUT = 0.0, 4.0            # the outlier component: N(0, sigma^2 + 4)
DISPLACED = {2: 8.0, 9: -10.0, 15: 12.0, 21: -15.0}      # in sigma


@functools.lru_cache(maxsize=None)
def _outlier_problem():
    """24 measurements of a constant 0.3 with error bars between 0.05 and
    0.15, four of them displaced by 8 to 15 of their sigma, drawn once."""
    rng = np.random.default_rng(2027)
    sigma = 0.05 + 0.1 * rng.random(24)
    data = MU_TRUE + sigma * rng.normal(size=24)
    for j, k in DISPLACED.items():
        data[j] = MU_TRUE + k * sigma[j]
    return data, sigma


def _mix(p):
    """The (n, 6) coefficients at outlier fractions ``p``: (c, a, f) = (1, 0,
    0), b and s fixed."""
    one = np.ones_like(p)
    return np.stack([one, 0 * one, 0 * one, p, B_OUT * one, S_OUT * one],
                    axis=1)


def _run_outlier():
    import torch
    from scipy import stats
    from nautilus_amd import GaussianOutlierLikelihood, Prior, Sampler
    data, sigma = _outlier_problem()
    prior = Prior()
    prior.add_parameter('mu', dist=stats.uniform(-1.0, 2.0))
    prior.add_parameter('p', dist=stats.uniform(0.0, P_MAX))
    assert prior.device                  # transformed on the GPU

    def model(x):
        one = torch.ones_like(x[:, 1])
        w = torch.stack([one, 0 * one, 0 * one, x[:, 1], B_OUT * one,
                         S_OUT * one], dim=1)
        return x[:, 0:1].expand(-1, 24), w

    like = GaussianOutlierLikelihood(model, data, sigma)
    s = Sampler(prior, like, pass_dict=False, n_live=1000, n_networks=2,
                vectorized=True, seed=0)
    s.run(n_eff=5000, discard_exploration=True)
    return like, s


def _simpson(n):
    w = np.ones(n)
    w[1:-1:2], w[2:-1:2] = 4.0, 2.0
    return w / 3.0


def _quadrature(n_mu, n_p):
    """log Z and the posterior means and standard deviations of (mu, p) by
    Simpson's rule on an (n_mu, n_p) grid of the twin over the prior's box
    (-1, 1) x (0, 1/2), whose density is 1."""
    from nautilus_amd import GaussianOutlierLikelihood
    data, sigma = _outlier_problem()
    like = GaussianOutlierLikelihood(identity, data, sigma)
    mu = np.linspace(-1.0, 1.0, n_mu)
    p = np.linspace(0.0, P_MAX, n_p)
    log_l = np.empty((n_mu, n_p))
    for k in range(n_p):
        log_l[:, k] = like.numpy_from_model(
            np.repeat(mu[:, None], 24, axis=1), _mix(np.full(n_mu, p[k])))
    shift = log_l.max()
    wgt = np.exp(log_l - shift) * np.outer(
        _simpson(n_mu) * (mu[1] - mu[0]), _simpson(n_p) * (p[1] - p[0]))
    z = wgt.sum()
    mean = np.array([(wgt.sum(axis=1) @ mu), (wgt.sum(axis=0) @ p)]) / z
    second = np.array([(wgt.sum(axis=1) @ mu**2),
                       (wgt.sum(axis=0) @ p**2)]) / z
    return np.log(z) + shift, mean, np.sqrt(second - mean**2)


def _quadrature_without_outliers(n_mu):
    """log Z of the same data under ``GaussianNoiseLikelihood`` with (c, a,
    f) = (1, 0, 0): one parameter, the prior density 1/2 on (-1, 1)."""
    from nautilus_amd import GaussianNoiseLikelihood
    data, sigma = _outlier_problem()
    like = GaussianNoiseLikelihood(identity, data, sigma)
    mu = np.linspace(-1.0, 1.0, n_mu)
    log_l = like.numpy_from_model(np.repeat(mu[:, None], 24, axis=1),
                                  np.tile([1.0, 0.0, 0.0], (n_mu, 1)))
    shift = log_l.max()
    return np.log(0.5 * (mu[1] - mu[0]) *
                  (_simpson(n_mu) @ np.exp(log_l - shift))) + shift


def test_sampler_recovers_mean_and_outlier_fraction():
    """Evidence and posterior means in the settings and the evidence band of
    test_sampler_recovers_mean_and_jitter (test_noise_likelihood_gpu.py),
    against quadrature; and the evidence without the outlier component is
    lower, which is what the model is for."""
    log_z, mean, sd = _quadrature(3201, 201)
    coarse = _quadrature(1601, 101)[0]
    print('log Z by quadrature %.6f, on half the grid %.6f' % (log_z, coarse))
    assert abs(log_z - coarse) < 1e-4
    plain = _quadrature_without_outliers(3201)
    assert abs(plain - _quadrature_without_outliers(1601)) < 1e-4
    print('log Z without the outlier component %.3f' % plain)
    assert plain < log_z - 10.0
    like, s = _run_outlier()
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
    # the four displaced measurements are the outliers at the posterior mean
    resp = like.numpy_responsibilities(np.full((1, 24), mean[0]),
                                       _mix(mean[1:2]))[0]
    assert sorted(np.flatnonzero(resp > 0.5)) == sorted(DISPLACED)
    _, again = _run_outlier()
    assert again.log_z == s.log_z and again.n_like == s.n_like
