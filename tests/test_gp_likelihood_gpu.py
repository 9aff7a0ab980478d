"""The fused device Gaussian-process likelihood (``nb_gp_loglike``,
nautilus_amd/csrc/nb_gp.hip) against the defining formula in ``np.longdouble``
under a derived error bound, its bit-for-bit independence of the batch, its
NaN rules, and end to end through ``Sampler``.  The problems, the reference
and the bound (``budget``, with its derivation) live in test_gp_likelihood.py,
which holds the numpy twin to them without a GPU."""

import functools

import numpy as np
import pytest

from test_gp_likelihood import (EDGE_TEST_P, EPS, MODES, P_ALL, ROW_TEST,
                                SHAPES, case_budget, check_classes, expected,
                                fixed_covariance_problem, identity, make,
                                problem, row_problem, sum_of_budgets,
                                white_noise_problem)

pytestmark = pytest.mark.gpu


def _mode(mode):
    from nautilus_amd import device
    return device.GP_HYPER if mode == 'hyper' else device.GP_FULL


def _cuda(*arrays):
    import torch
    return [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in arrays]


def test_shapes_cover_both_sides_of_every_launcher_boundary():
    from nautilus_amd import device
    shapes = [device.gp_launch_shape(p) for p in range(1, 129)]
    changes = [p for p in range(1, 128) if shapes[p - 1] != shapes[p]]
    assert changes == [16, 32, 48, 64, 80, 96, 112]
    for p in changes:
        assert p in P_ALL and p + 1 in P_ALL
    assert 1 in P_ALL and 128 in P_ALL
    assert [s[0] for s in shapes[15::16]] == list(range(1, 9))
    assert sorted({s[1] for s in shapes}) == [1, 2, 4]
    for p in (0, 129):
        with pytest.raises(ValueError):
            device.gp_launch_shape(p)


@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('p, n, kernel, rot', SHAPES)
def test_values(p, n, kernel, rot, mode):
    """|device - long double| <= budget in every row (the budget is derived
    in test_gp_likelihood.budget)."""
    import torch
    check_classes(p, n, mode, kernel, rot)
    t, d, sigma, m, cov = problem(p, n, mode, kernel, rot)
    want = expected(p, n, mode, kernel, rot).out
    tol = case_budget(p, n, mode, kernel, rot)
    raw = make(t, d, sigma, mode, kernel)
    mt, ct = _cuda(m, cov)
    out = raw.from_model(mt, ct)
    assert out.is_cuda and out.dtype == torch.float64 and out.shape == (n,)
    got = out.cpu().numpy()
    err = np.abs(got - want)
    print('P = %d, n = %d, %s, %s: largest used fraction of the bound %.3g, '
          'of its factorisation part %.3g' % (
              p, n, kernel, mode, (err / tol.total).max(),
              (err / tol.factorisation).max()))
    assert np.all(np.isfinite(got))
    assert np.all(err <= tol.total), (err / tol.total).max()
    # the constant joins with one subtraction: log_norm - sum / 2
    like = make(t, d, sigma, mode, kernel, normalised=True)
    assert like.log_norm == -0.5 * p * np.log(2 * np.pi)
    assert np.array_equal(like.from_model(mt, ct).cpu().numpy(),
                          like.log_norm + got)


@pytest.mark.parametrize('mode, p', [(mode, p) for mode in MODES
                                     for p in ROW_TEST[mode][0]])
def test_rows_bit_for_bit(p, mode):
    """A row's bits are those it has alone, inside batches of 17 and of many
    at different positions, with m and the covariance input each in place
    inside a wider tensor, on any stream."""
    import torch
    n = ROW_TEST[mode][1]
    t, d, sigma, m, cov = row_problem(p, n, mode)
    like = make(t, d, sigma, mode, 'matern32', normalised=True)
    width = 3 if mode == 'hyper' else p * p
    big, cbig = _cuda(m, cov)
    full = like.from_model(big, cbig)
    assert bool(torch.isfinite(full).all())
    for off in (0, 1, 777, 4080):
        off = min(off, n - 17)
        sub, csub = big[off:off + 17], cbig[off:off + 17]
        assert sub.data_ptr() == big.data_ptr() + off * p * 8   # a view
        assert csub.data_ptr() == cbig.data_ptr() + off * width * 8
        assert torch.equal(like.from_model(sub, csub), full[off:off + 17]), off
        for r in (off, off + 16):
            assert torch.equal(like.from_model(big[r:r + 1], cbig[r:r + 1]),
                               full[r:r + 1])
    # the same rows at other positions of a batch
    perm = torch.from_numpy(np.random.default_rng(p).permutation(n)).cuda()
    assert torch.equal(like.from_model(big[perm], cbig[perm]), full[perm])
    assert like.from_model(big[:0], cbig[:0]).shape == (0,)
    # slices of wider tensors, m and the covariance input independently
    rng = np.random.default_rng(p)
    wide = torch.from_numpy(rng.normal(size=(n, p + 5))).cuda()
    wide[:, 2:2 + p] = big
    view = wide[:, 2:2 + p]
    assert view.data_ptr() == wide.data_ptr() + 2 * 8
    assert view.stride() == (p + 5, 1)
    if mode == 'hyper':
        cwide = torch.from_numpy(rng.normal(size=(n, 6))).cuda()
        cwide[:, 1:4] = cbig
        cview = cwide[:, 1:4]
        assert cview.stride() == (6, 1)
        pad = 6
    else:
        # p + 1 matrices' worth of rows per point, the covariance from row 1
        # on: an odd distance between the matrices at odd P
        cwide = torch.from_numpy(rng.normal(size=(n, p + 2, p, p))).cuda()
        cwide[:, 1] = cbig
        cview = cwide[:, 1]
        assert cview.stride() == ((p + 2) * p * p, p, 1)
        pad = (p + 2) * p * p
    assert cview.data_ptr() == cwide.data_ptr() + (8 if mode == 'hyper'
                                                   else p * p * 8)
    assert torch.equal(like.from_model(view, cbig), full)
    assert torch.equal(like.from_model(big, cview), full)
    assert torch.equal(like.from_model(view, cview), full)
    if mode == 'full':
        # an odd row stride takes the loads one double at a time
        flat = torch.from_numpy(rng.normal(size=(n, p * p + 1))).cuda()
        flat[:, 1:] = cbig.reshape(n, p * p)
        odd = flat[:, 1:].unflatten(1, (p, p))
        assert odd.data_ptr() == flat.data_ptr() + 8
        assert odd.stride() == (p * p + 1, p, 1)
        assert torch.equal(like.from_model(big, odd), full)
    table = like._table()
    code = _mode(mode)
    c2 = cview.reshape(n, width) if mode == 'hyper' else \
        cview.as_strided((n, width), (pad, 1))
    assert c2.data_ptr() == cview.data_ptr()
    assert torch.equal(table.loglike(view, c2, code, ld=p + 5, ld_cov=pad),
                       full)
    assert torch.equal(table.loglike(view[5:22], c2[5:22], code), full[5:22])
    # a stream of its own
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        other = like.from_model(big, cbig)
        one = like.from_model(view[9:10], cview[9:10])
    stream.synchronize()
    assert torch.equal(other, full) and torch.equal(one, full[9:10])


BAD_HYPER = [(0, -1e-300), (0, float('nan')), (0, float('inf')),
             (0, float('-inf')), (1, 0.0), (1, -2.0), (1, float('nan')),
             (1, float('inf')), (2, -1e-300), (2, float('nan')),
             (2, float('inf'))]


@pytest.mark.parametrize('p', EDGE_TEST_P)
def test_edge_rows_hyper(p):
    """One NaN cause at a time in row 7 of a batch of 17: that row is NaN and
    the other sixteen keep their bits."""
    import torch
    kernel = 'matern52'
    t, d, sigma, m, h = problem(p, 17, 'hyper', kernel)
    like = make(t, d, sigma, 'hyper', kernel, normalised=True)
    cm, ch = _cuda(m, h)
    want = like.from_model(cm, ch)
    assert bool(torch.isfinite(want).all())
    keep = torch.ones(17, dtype=torch.bool, device='cuda')
    keep[7] = False

    def check(dm, dh, what):
        out = like.from_model(dm, dh)
        assert bool(torch.isnan(out[7])), what
        assert torch.equal(out[keep], want[keep]), what
        twin = like.numpy_from_model(dm.cpu().numpy(), dh.cpu().numpy())
        assert np.array_equal(np.isnan(twin), torch.isnan(out).cpu().numpy())

    for col, value in BAD_HYPER:
        dh = ch.clone()
        dh[7, col] = value
        check(cm, dh, (col, value))
    for col, value in ((0, float('nan')), (p - 1, float('inf')),
                       (p // 2, float('-inf'))):
        dm = cm.clone()
        dm[7, col] = value
        check(dm, ch, ('m', col, value))
    # not positive definite: the jitter cannot be negative, but sigma_j = 0 in
    # a column, a = 0 and s = 0 leave a zero on the diagonal
    assert np.any(sigma == 0.0)
    dh = ch.clone()
    dh[7] = torch.tensor([0.0, 1.0, 0.0])
    check(cm, dh, 'zero pivot')
    # a = 0 is legal: independent Gaussians with variances sigma^2 + s
    rows = np.flatnonzero(h[:, 0] == 0.0)
    assert len(rows) >= 4
    v = (sigma.astype(np.longdouble)**2 + h[rows, 2].astype(
        np.longdouble)[:, None])
    r = m[rows].astype(np.longdouble) - d.astype(np.longdouble)
    white = (like.log_norm - 0.5 * (r * r / v + np.log(v)).sum(
        axis=1)).astype(float)
    tol = case_budget(p, 17, 'hyper', kernel).total[rows] + \
        EPS * np.abs(white)
    assert np.all(np.abs(want.cpu().numpy()[rows] - white) <= tol)


@pytest.mark.parametrize('p', EDGE_TEST_P)
def test_edge_rows_full(p):
    import torch
    t, d, sigma, m, c = problem(p, 17, 'full', 'sqexp')
    like = make(None, d, sigma, 'full', normalised=True)
    cm, cc = _cuda(m, c)
    want = like.from_model(cm, cc)
    assert bool(torch.isfinite(want).all())
    keep = torch.ones(17, dtype=torch.bool, device='cuda')
    keep[7] = False

    def check(dm, dc, what):
        out = like.from_model(dm, dc)
        assert bool(torch.isnan(out[7])), what
        assert torch.equal(out[keep], want[keep]), what

    for (j, k), value in (((0, 0), float('nan')), ((p - 1, 0), float('inf')),
                          ((p - 1, p - 1), float('-inf')),
                          ((p // 2, p // 3), float('nan'))):
        dc = cc.clone()
        dc[7, j, k] = value
        check(cm, dc, ('C', j, k, value))
    dm = cm.clone()
    dm[7, p - 1] = float('nan')
    check(dm, cc, 'm')
    # one eigenvalue of K set to -1, and an exactly singular K (its first and
    # last rows and columns are equal, and every step of it is exact)
    k7 = c[7] + np.diag(sigma**2)
    w, v = np.linalg.eigh(k7)
    w[len(w) // 2] = -1.0
    indefinite = (v * w) @ v.T
    dc = cc.clone()
    dc[7] = torch.from_numpy(indefinite - np.diag(sigma**2)).cuda()
    check(cm, dc, 'an eigenvalue of -1')
    zero_sigma = make(None, d, None, 'full', normalised=True)
    want0 = zero_sigma.from_model(cm, cc)
    singular = np.eye(p)
    singular[0, 0] = singular[p - 1, 0] = singular[0, p - 1] = \
        singular[p - 1, p - 1] = 4.0           # the last pivot is 4 - 2 * 2
    dc = cc.clone()
    dc[7] = torch.from_numpy(singular).cuda()
    out = zero_sigma.from_model(cm, dc)
    assert bool(torch.isnan(out[7])) and torch.equal(out[keep], want0[keep])
    # the upper triangle is not read
    dc = cc.clone()
    upper = torch.triu(torch.ones(p, p, dtype=torch.bool, device='cuda'), 1)
    dc[:, upper] = float('nan')
    assert torch.equal(like.from_model(cm, dc), want)


def test_one_handle_on_two_streams():
    import torch
    t, d, sigma, m, h = problem(65, 130, 'hyper', 'exp')
    ht, x = _cuda(h, m)
    from nautilus_amd import GaussianProcessLikelihood
    like = GaussianProcessLikelihood(lambda x: (x, ht), t, d, sigma,
                                     kernel='exp')
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
            device.GPTable(*args, **kw)
        assert str(err.value) != 'nautilus_hip: '
        return err.value.code

    d = np.array([0.5, -2.0, 5.5])
    dist = np.abs(np.subtract.outer(np.arange(3.0), np.arange(3.0)))
    assert device.GP is device.GPTable
    assert device.GPTable(d).n_data == 3
    assert device.GPTable(d, np.r_[0.0, 1.0, 4.0], dist, kernel='matern52',
                          log_norm=-3.0).n_data == 3
    assert code(np.zeros(0)) == _lib.ERR_ARG
    assert code(np.zeros(129)) == _lib.ERR_ARG
    assert code(np.r_[1.0, np.nan, 1.0]) == _lib.ERR_ARG
    for bad in (-1e-300, np.nan, np.inf):
        assert code(d, np.r_[0.0, bad, 1.0]) == _lib.ERR_ARG
    assert code(d, log_norm=np.nan) == _lib.ERR_ARG
    for j, k, bad in ((2, 1, 5.0), (0, 0, 1.0), (1, 0, np.nan)):
        wrong = dist.copy()
        wrong[j, k] = bad
        if np.isnan(bad):
            wrong[k, j] = bad
        assert code(d, None, wrong) == _lib.ERR_ARG
    lib = _lib.load()
    h = ctypes.c_void_p()

    def raw_refused(fn, *args):
        # another entry's message first: the text checked below is this call's
        assert lib.nb_poisson_create(0, None, None, None, 0.0,
                                     None) == _lib.ERR_ARG
        assert b'Poisson' in lib.nb_last_error()
        assert fn(*args) == _lib.ERR_ARG
        assert b'Gaussian-process likelihood' in lib.nb_last_error()

    dp = d.ctypes.data_as(_lib.c_double_p)
    raw_refused(lib.nb_gp_create, 3, None, None, None, 0, 0.0, ctypes.byref(h))
    raw_refused(lib.nb_gp_create, 3, dp, None, None, 0, 0.0, None)
    raw_refused(lib.nb_gp_create, 3, dp, None, None, 4, 0.0, ctypes.byref(h))
    raw_refused(lib.nb_gp_create, 3, dp, None, None, -1, 0.0, ctypes.byref(h))
    table = device.GPTable(d, np.ones(3), dist)
    bare = device.GPTable(d, np.ones(3))
    m = torch.ones(4, 3, dtype=torch.float64, device='cuda')
    h3 = torch.ones(4, 3, dtype=torch.float64, device='cuda')
    c9 = torch.eye(3, dtype=torch.float64, device='cuda').reshape(
        1, 9).repeat(4, 1)
    hyper, full = device.GP_HYPER, device.GP_FULL

    def refused(tab, *args, **kw):
        with pytest.raises(_lib.NativeError) as err:
            tab.loglike(*args, **kw)
        assert err.value.code == _lib.ERR_ARG
        assert 'Gaussian-process likelihood' in str(err.value)
        return str(err.value)

    # an unknown mode; hyper mode on a handle without distances
    assert 'mode NB_GP_HYPER or NB_GP_FULL' in refused(table, m, h3, 2)
    refused(table, m, h3, -1)
    assert 'needs a handle created with dist' in refused(bare, m, h3, hyper)
    assert bare.loglike(m, c9, full).shape == (4,)
    # ld and ld_cov count from the second row on
    assert 'ld_cov >= 3' in refused(table, m, h3, hyper, ld=2)
    refused(table, m, h3, hyper, ld_cov=2)
    assert 'ld_cov >= 9' in refused(table, m, c9, full, ld_cov=8)
    refused(table, m, c9, full, ld=2)
    want = table.loglike(m, h3, hyper)
    assert want.shape == (4,) and bool(torch.isfinite(want).all())
    assert torch.equal(table.loglike(m, h3, hyper, ld=3, ld_cov=3), want)
    assert torch.equal(table.loglike(m[:1], h3[:1], hyper, ld=0, ld_cov=0),
                       want[:1])
    assert torch.equal(table.loglike(m[:1], c9[:1], full, ld=0, ld_cov=0),
                       table.loglike(m, c9, full)[:1])
    # NULL pointers with n > 0, and none needed for n = 0
    out = torch.empty(4, dtype=torch.float64, device='cuda')
    ptrs = dict(h=table._h, m=m.data_ptr(), c=h3.data_ptr(),
                out=out.data_ptr())
    for null in ('h', 'm', 'c', 'out'):
        a = dict(ptrs)
        a[null] = None
        raw_refused(lib.nb_gp_loglike, a['h'], hyper, a['m'], 3, a['c'], 3, 4,
                    a['out'], None)
    raw_refused(lib.nb_gp_loglike, table._h, hyper, m.data_ptr(), 3,
                h3.data_ptr(), 3, -1, out.data_ptr(), None)
    assert lib.nb_gp_loglike(table._h, hyper, None, 3, None, 3, 0, None,
                             None) == 0
    assert lib.nb_gp_loglike(table._h, full, None, 0, None, 0, 0, None,
                             None) == 0
    assert lib.nb_gp_destroy(None) == 0
    # shapes that do not fit together never reach the library
    with pytest.raises(ValueError):
        device.GPTable(d, np.ones(4))
    with pytest.raises(ValueError):
        device.GPTable(d, None, np.zeros((3, 4)))
    with pytest.raises(ValueError):
        device.GPTable(d, kernel='periodic')
    with pytest.raises(ValueError):
        table.loglike(m, h3[:3], hyper)


def test_white_noise_against_the_data_vector_likelihood():
    """a = 0, s = 0 is ``GaussianDataLikelihood(sigma=...)``, both on the
    device, to the sum of the two budgets."""
    from nautilus_amd import GaussianDataLikelihood
    t, d, sigma, m, h = white_noise_problem()
    like = make(t, d, sigma, 'hyper', normalised=True)
    mt, ht = _cuda(m, h)
    got = like.from_model(mt, ht).cpu().numpy()
    want = GaussianDataLikelihood(identity, d, sigma=sigma).from_model(
        mt).cpu().numpy()
    tol = sum_of_budgets(len(d), like.dist, d, sigma, m, h, 'hyper') + \
        4 * EPS * np.abs(want)
    used = np.abs(got - want) / tol
    print('largest used fraction of the two budgets %.3g' % used.max())
    assert np.all(used <= 1.0), used.max()


def test_fixed_covariance_against_the_data_vector_likelihood():
    """One C for every row is ``GaussianDataLikelihood(cov=C + diag(sigma^2))``,
    whose constant includes the determinant; both on the device."""
    from nautilus_amd import GaussianDataLikelihood
    d, sigma, m, c = fixed_covariance_problem()
    n, p = m.shape
    cov = np.broadcast_to(c, (n, p, p)).copy()
    like = make(None, d, sigma, 'full', normalised=True)
    mt, ct = _cuda(m, cov)
    got = like.from_model(mt, ct).cpu().numpy()
    want = GaussianDataLikelihood(
        identity, d, cov=c + np.diag(sigma**2)).from_model(mt).cpu().numpy()
    tol = sum_of_budgets(p, None, d, sigma, m, cov, 'full') + \
        4 * EPS * np.abs(want)
    used = np.abs(got - want) / tol
    print('largest used fraction of the two budgets %.3g' % used.max())
    assert np.all(used <= 1.0), used.max()


# ---------------------------------------------------------- through Sampler

GP_TRUE = (1.0, 1.5, 0.01)                    # a, l, s
GP_SIGMA = 0.05
GP_BOX = ((0.05, 20.0), (0.1, 20.0), (1e-4, 1.0))
# log Z of five runs that differ in the seed alone (0 .. 4), on an MI355X
LOG_Z_SEEDS = (-17.9168, -17.9195, -17.8985, -17.9124, -17.9058)


@functools.lru_cache(maxsize=None)
def _process_problem():
    """24 points of a zero-mean Matern-3/2 process on sorted uniform locations
    in [0, 10] with error bars of 0.05, drawn once."""
    from nautilus_amd.likelihoods import gp_correlation
    rng = np.random.default_rng(2027)
    t = np.sort(rng.uniform(0, 10, size=24))
    a, l, s = GP_TRUE
    k = a * gp_correlation('matern32', np.abs(t[:, None] - t[None, :]) / l) + \
        (s + GP_SIGMA**2) * np.eye(24)
    return t, np.linalg.cholesky(k) @ rng.normal(size=24)


def _process_likelihood():
    import torch
    from nautilus_amd import GaussianProcessLikelihood
    t, data = _process_problem()

    def model(x):
        return torch.zeros(x.shape[0], 24, dtype=torch.float64,
                           device=x.device), x

    return GaussianProcessLikelihood(model, t, data, np.full(24, GP_SIGMA),
                                     kernel='matern32')


def _run_process(seed=0):
    from scipy import stats
    from nautilus_amd import Prior, Sampler
    prior = Prior()
    for name, (lo, hi) in zip('als', GP_BOX):
        prior.add_parameter(name, dist=stats.loguniform(lo, hi))
    assert prior.device                  # transformed on the GPU
    s = Sampler(prior, _process_likelihood(), pass_dict=False, n_live=1000,
                vectorized=True, seed=seed)
    s.run(n_eff=5000, discard_exploration=True)
    return s


@functools.lru_cache(maxsize=None)
def _quadrature(k):
    """log Z and the posterior means and standard deviations of (log a,
    log l, log s) by the midpoint rule on a k^3 grid over the prior box, in
    which the prior is uniform in the logarithms: the numpy twin at every
    node."""
    like = _process_likelihood()
    axes = [np.log(lo) + (np.arange(k) + 0.5) / k * np.log(hi / lo)
            for lo, hi in GP_BOX]
    grid = np.stack(np.meshgrid(*axes, indexing='ij'), axis=-1).reshape(-1, 3)
    log_l = np.concatenate([
        like.numpy_from_model(np.zeros((len(part), 24)), np.exp(part))
        for part in np.array_split(grid, max(1, len(grid) // 8192))])
    shift = log_l.max()
    w = np.exp(log_l - shift)
    mean = w @ grid / w.sum()
    sd = np.sqrt(w @ (grid - mean)**2 / w.sum())
    return np.log(w.mean()) + shift, mean, sd


def test_sampler_recovers_the_hyper_parameters():
    """Evidence and posterior means of log a and log l against quadrature.
    The band on log Z is four standard deviations of LOG_Z_SEEDS, five runs
    on an MI355X that differ in the seed alone:
        -17.9168, -17.9195, -17.8985, -17.9124, -17.9058
    (standard deviation 0.0085, band 0.034; the quadrature gives -17.9086).
    The quadrature is refined from 24^3 to 36^3 nodes and may move by a tenth
    of the band at most."""
    band = 4 * np.std(LOG_Z_SEEDS, ddof=1)
    coarse, fine = _quadrature(24), _quadrature(36)
    log_z, mean, sd = fine
    print('quadrature log Z = %.5f (24^3: %.5f), band %.4f' % (
        log_z, coarse[0], band))
    assert abs(log_z - coarse[0]) < 0.1 * band
    s = _run_process()
    print('log Z = %.4f, quadrature %.4f, n_like = %d, n_eff = %.0f' % (
        s.log_z, log_z, s.n_like, s.n_eff))
    assert abs(s.log_z - log_z) < band
    pts, log_w, _ = s.posterior()
    wgt = np.exp(log_w - np.max(log_w))
    got = (wgt @ np.log(pts) / wgt.sum())[:2]
    tol = 4 * sd[:2] / np.sqrt(s.n_eff)
    print('posterior mean - quadrature mean in units of the tolerance:',
          (got - mean[:2]) / tol, 'means', mean, 'sd', sd)
    assert np.all(np.abs(got - mean[:2]) < tol)
    again = _run_process()
    assert again.log_z == s.log_z and again.n_like == s.n_like
