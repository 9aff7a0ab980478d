"""Device prior transform for uniform, normal, log-uniform, log-normal,
half-normal and truncated normal parameters (``nb_prior_table_transform``)
against what the reference's ``Prior`` computes: scipy's ``dist.isf(1 - u)``
on the host, through this package's own numpy path."""

import numpy as np
import pytest
from scipy import stats
from scipy.special import ndtri

from conftest import load_golden

pytestmark = pytest.mark.gpu

EPS = 2.0**-52
LOGUNIFORM = [(1e-3, 10.0), (1.0, 2.0), (1e-8, 1e8)]
LOGNORM = [0.1, 0.7, 2.5]
TRUNCNORM = [(-1.0, 2.0), (2.0, 6.0), (-np.inf, 1.0), (5.0, np.inf),
             (-8.0, -6.0), (-3.0, 3.0), (0.0, np.inf)]
# further out than the masses of the interval can be formed: log space
FAR = [(40.0, np.inf), (36.0, 37.0), (-np.inf, -38.0), (-101.0, -100.0)]
KINDS = ['uniform', 'norm', 'loguniform', 'lognorm', 'halfnorm', 'truncnorm']


def _spec(kind, j):
    """(kind, frozen distribution, what the check needs) of free parameter
    ``j``; the shapes cycle through the lists above."""
    if kind == 'uniform':
        loc, scale = -3.0 + 0.37 * j, 0.1 + 1.3 * (j % 7)
        return kind, stats.uniform(loc=loc, scale=scale), None
    if kind == 'norm':
        return kind, stats.norm(loc=2.0 - 0.1 * j, scale=0.5 + 0.01 * j), None
    if kind == 'loguniform':
        a, b = LOGUNIFORM[(j // 6) % 3]
        gen = stats.reciprocal if j % 2 else stats.loguniform
        return kind, gen(a, b, scale=1.0 + 0.25 * (j % 5)), (a, b)
    if kind == 'lognorm':
        s = LOGNORM[(j // 6) % 3]
        return kind, stats.lognorm(s, scale=0.5 + 0.5 * (j % 4)), s
    if kind == 'halfnorm':
        return kind, stats.halfnorm(loc=0.25 * (j % 3), scale=1.0 + 0.1 * j), \
            None
    a, b = TRUNCNORM[(j // 6) % 7]
    return kind, stats.truncnorm(a, b), (a, b)


def _prior(d, first=0):
    """``d`` free parameters that cycle through the six kinds starting at
    ``first``, a fixed key after the first and a tied key after every fourth
    free parameter (and one tied to the fixed key at the end)."""
    from nautilus_amd import Prior
    prior, specs = Prior(), []
    for j in range(d):
        spec = _spec(KINDS[(first + j) % 6], first + j)
        specs.append(spec)
        prior.add_parameter('p%d' % j, dist=spec[1])
        if j == 0:
            prior.add_parameter('fixed', dist=1.5)
        if j % 4 == 3:
            prior.add_parameter('tied%d' % j, dist='p%d' % (j - 2))
    prior.add_parameter('tied_fixed', dist='fixed')
    return prior, specs


def _unit_points(d):
    """The inputs of test_prior_on_device: 5000 rows of default_rng(0), of
    which the first three are the edge values."""
    u = np.random.default_rng(0).random((5000, d))
    u[0], u[1], u[2] = 0.0, 1e-300, 1 - 2.0**-53
    return u


def _scipy_dev():
    g = load_golden('truncnorm_exact')
    dev = {tuple(pair): dev for pair, dev in zip(g['pairs'], g['scipy_dev'])}
    dev.update({tuple(pair): dev for pair, dev in zip(g['far_pairs'],
                                                      g['far_scipy_dev'])})
    return dev


def _check_column(kind, info, u, got, want, name):
    """One free parameter against scipy, in the band of its kind."""
    q = 1.0 - u
    odd = ~np.isfinite(want)
    assert np.array_equal(got[odd], want[odd]), name     # non-finite as scipy
    if kind == 'uniform':
        assert np.array_equal(got, want), name
        return
    if kind in ('norm', 'halfnorm'):
        assert np.allclose(got, want, rtol=1e-12, atol=1e-13), name
        return
    ok = ~odd
    err = np.abs(got[ok] - want[ok])
    if kind == 'lognorm':
        # x = exp(s z): the band of z (rtol 1e-12, atol 1e-13) times s
        z = ndtri(q[ok])
        fin = np.isfinite(z)
        assert np.array_equal(got[ok][~fin], want[ok][~fin]), name
        rtol = info * (1e-12 * np.abs(z[fin]) + 1e-13) + 4 * EPS
        worst = np.max(err[fin] / (rtol * np.abs(want[ok][fin])))
        print('%s lognorm s=%g: worst error / band = %.3f' % (name, info,
                                                              worst))
        assert worst <= 1.0, name
    elif kind == 'loguniform':
        # log and exp good to 2 ulp each, t up to max(|log a|, |log b|)
        a, b = info
        rtol = 8 * EPS * (1 + abs(np.log(a)) + abs(np.log(b)))
        worst = np.max(err / np.abs(want[ok])) / rtol
        print('%s loguniform (%g, %g): worst error / band = %.3f, '
              'max relative error %.3e' % (name, a, b, worst, worst * rtol))
        assert worst <= 1.0, name
    else:
        # scipy itself is only good inside [1e-6, 1 - 1e-6] (the fixture
        # records how good): 4 x its deviation + 1e-12, in units of
        # 0.1 + |x| (rtol 1e-12 with atol 1e-13)
        a, b = info
        inside = (u >= 1e-6) & (u <= 1 - 1e-6)
        band = (4 * _scipy_dev()[info] + 1e-12) * (0.1 + np.abs(want[inside]))
        worst = np.max(np.abs(got[inside] - want[inside]) / band)
        print('%s truncnorm (%g, %g): worst deviation from scipy / band = '
              '%.3f' % (name, a, b, worst))
        assert worst <= 1.0, name
        _check_truncnorm_range(u, got, a, b, 0.0, 1.0, name)


def _check_truncnorm_range(u, got, a, b, loc, scale, name):
    """Over all of [0, 1), edge rows included: inside the support,
    non-decreasing in u, and finite -- except that where 1 - u rounds to 1
    (u = 0 and u = 1e-300) the quantile of an interval that is unbounded
    below IS -inf, for scipy as well."""
    lo, hi = loc + a * scale, loc + b * scale
    assert np.all((got >= lo) & (got <= hi)), name
    ordered = got[np.argsort(u, kind='stable')]
    assert np.all(ordered[1:] >= ordered[:-1]), name
    at_zero = (1.0 - u) == 1.0
    assert np.all(np.isfinite(got[~at_zero])), name
    if np.isfinite(a):
        assert np.all(np.isfinite(got)), name
    else:
        assert np.all(got[at_zero] == -np.inf), name


@pytest.mark.parametrize('d,first', [(1, 0), (1, 1), (1, 2), (1, 3), (1, 4),
                                     (1, 5), (7, 0), (50, 0), (128, 0),
                                     (50, 3), (127, 2)])
def test_values_against_scipy(d, first):
    """Both layouts against scipy at d = 1 (each kind), 7, 50, 128 free
    parameters (and odd / shifted variants, so that every shape of every
    kind and all seven truncnorm intervals occur)."""
    import torch
    prior, specs = _prior(d, first)
    assert prior.device and prior.dimensionality() == d
    u = _unit_points(d)
    want = prior.unit_to_physical(u)
    u_dev = torch.from_numpy(u).cuda()
    rows = prior.unit_to_physical(u_dev)
    assert rows.shape == (5000, d) and rows.is_contiguous()
    got = rows.cpu().numpy()
    for j, (kind, _, info) in enumerate(specs):
        _check_column(kind, info, u[:, j], got[:, j], want[:, j],
                      'd=%d column %d' % (d, j))
    # column-major: the same numbers, one contiguous row per key
    dic = prior.unit_to_dictionary(u_dev)
    host = prior.unit_to_dictionary(u)
    assert list(dic) == prior.keys
    base = {v.untyped_storage().data_ptr() for v in dic.values()}
    assert len(base) == 1                     # views of ONE allocation
    for key, value in dic.items():
        assert value.shape == (5000,) and value.is_contiguous(), key
        assert value.is_cuda and value.dtype == torch.float64
    for j in range(d):
        assert torch.equal(dic['p%d' % j], rows[:, j]), j
    assert torch.all(dic['fixed'] == 1.5) and torch.all(
        dic['tied_fixed'] == 1.5)
    for key, dist in zip(prior.keys, prior.dists):
        if isinstance(dist, str):
            assert torch.equal(dic[key], dic[dist]), key
        assert dic[key].cpu().numpy().shape == host[key].shape


def test_truncnorm_against_exact_values():
    """The seven intervals, and four far in the tails (log space), on the
    fixture's 2000 points of [1e-6, 1 - 1e-6]:
    within 4 x scipy's recorded deviation + 1e-12 of scipy, and within the
    project's band for normal quantiles (rtol 1e-12, atol 1e-13) of the exact
    values (60-digit mpmath, tests/golden/make_golden_truncnorm.py)."""
    import torch
    from nautilus_amd import Prior
    g = load_golden('truncnorm_exact')
    u = g['u']
    pairs = np.concatenate([g['pairs'], g['far_pairs']])
    exact_all = np.concatenate([g['exact'], g['far_exact']])
    scipy_dev = np.concatenate([g['scipy_dev'], g['far_scipy_dev']])
    assert [tuple(p) for p in pairs] == TRUNCNORM + FAR
    prior = Prior()
    for k, (a, b) in enumerate(pairs):
        prior.add_parameter('t%d' % k, dist=stats.truncnorm(a, b))
    points = np.repeat(u[:, None], len(pairs), axis=1)
    want = prior.unit_to_physical(points)
    got = prior.unit_to_physical(torch.from_numpy(points).cuda()).cpu().numpy()
    failed = []
    for k, (a, b) in enumerate(pairs):
        exact = exact_all[k]
        band = (4 * scipy_dev[k] + 1e-12) * (0.1 + np.abs(want[:, k]))
        vs_scipy = np.max(np.abs(got[:, k] - want[:, k]) / band)
        err = np.abs(got[:, k] - exact)
        vs_exact = np.max(err / (1e-13 + 1e-12 * np.abs(exact)))
        worst = np.argmax(err / (1e-13 + 1e-12 * np.abs(exact)))
        print('truncnorm (%g, %g): from scipy %.3f of its band, from exact '
              '%.3e of rtol 1e-12 / atol 1e-13 (|error| %.3e at u = %r)' %
              (a, b, vs_scipy, vs_exact, err[worst], u[worst]))
        if vs_scipy > 1.0 or vs_exact > 1.0:
            failed.append((a, b, vs_scipy, vs_exact))
        assert np.all(got[1:, k] >= got[:-1, k])        # u is sorted
        assert np.all((got[:, k] >= a) & (got[:, k] <= b))
    assert not failed, failed


def test_truncnorm_with_loc_and_scale():
    """loc / scale on a truncated normal: inside [loc + a scale, loc + b
    scale], monotone, and as close to scipy as the standard one, x = z scale +
    loc carrying the band of z times scale plus two roundings."""
    import torch
    from nautilus_amd import Prior
    dev = _scipy_dev()
    loc, scale = 0.5, 2.0
    prior = Prior()
    pairs = TRUNCNORM + FAR
    for k, (a, b) in enumerate(pairs):
        prior.add_parameter('t%d' % k,
                            dist=stats.truncnorm(a, b, loc=loc, scale=scale))
    u = _unit_points(len(pairs))
    want = prior.unit_to_physical(u)
    got = prior.unit_to_physical(torch.from_numpy(u).cuda()).cpu().numpy()
    for k, (a, b) in enumerate(pairs):
        _check_truncnorm_range(u[:, k], got[:, k], a, b, loc, scale, (a, b))
        inside = (u[:, k] >= 1e-6) & (u[:, k] <= 1 - 1e-6)
        z = np.abs(want[:, k] - loc) / scale
        z = z[inside]
        band = scale * (4 * dev[(a, b)] + 1e-12) * (0.1 + z) + \
            2 * EPS * (z * scale + np.abs(want[inside, k]))
        assert np.all(np.abs(got[inside, k] - want[inside, k]) <= band), (a, b)


def test_one_table_serves_two_streams():
    import torch
    prior, _ = _prior(50)
    u = torch.from_numpy(_unit_points(50)).cuda()
    ref = prior.unit_to_physical(u)
    handle = prior._device_handle()
    torch.cuda.synchronize()
    outs = []
    for _ in range(2):
        stream = torch.cuda.Stream()
        with torch.cuda.stream(stream):
            outs.append((prior.unit_to_physical(u),
                         prior.unit_to_dictionary(u)))
        assert prior._device_handle() is handle
    torch.cuda.synchronize()
    for rows, dic in outs:
        assert torch.equal(rows, ref)
        assert torch.equal(dic['p7'], ref[:, 7])


def test_ragged_and_small_batches():
    """Row counts around the kernel's block of 64 rows, odd widths: equal to
    the same rows inside a large batch, bit for bit."""
    import torch
    for d in (1, 7, 127):
        prior, _ = _prior(d, 2)
        u = torch.from_numpy(_unit_points(d)[3:]).cuda()
        ref = prior.unit_to_physical(u)
        for n in (1, 2, 63, 64, 65, 129, 1000):
            part = u[5:5 + n]               # odd offsets: 8-byte alignment
            assert torch.equal(prior.unit_to_physical(part), ref[5:5 + n])
            dic = prior.unit_to_dictionary(part)
            assert torch.equal(dic['p%d' % (d - 1)], ref[5:5 + n, d - 1])
            assert dic['fixed'].shape == (n,) and bool(
                (dic['fixed'] == 1.5).all())
        assert prior.unit_to_physical(u[:0]).shape == (0, d)


def test_old_entry_still_refuses_other_kinds():
    import torch
    from nautilus_amd import _lib, device
    u = torch.rand(10, 1, dtype=torch.float64, device='cuda')
    with pytest.raises(_lib.NativeError) as err:
        device.prior_transform(u, [2], [0.0], [1.0])
    assert err.value.code == _lib.ERR_UNSUPPORTED


def test_table_arguments_are_checked():
    from nautilus_amd import _lib, device

    def create(kind, scale=1.0, s0=0.0, s1=0.0, column=0):
        return device.PriorTable([kind], [0.0], [scale], [s0], [s1], [column],
                                 [0.0])
    for args, code in [
            (dict(kind=6), _lib.ERR_UNSUPPORTED),
            (dict(kind=0, scale=0.0), _lib.ERR_ARG),
            (dict(kind=2, s0=0.0, s1=1.0), _lib.ERR_ARG),
            (dict(kind=2, s0=2.0, s1=1.0), _lib.ERR_ARG),
            (dict(kind=3, s0=0.0), _lib.ERR_ARG),
            (dict(kind=5, s0=1.0, s1=1.0), _lib.ERR_ARG),
            (dict(kind=5, s0=1e200, s1=np.inf), _lib.ERR_UNSUPPORTED),
            (dict(kind=0, column=1), _lib.ERR_ARG)]:
        with pytest.raises(_lib.NativeError) as err:
            create(**args)
        assert err.value.code == code, args
    with pytest.raises(_lib.NativeError) as err:
        device.PriorTable([0] * 129, [0.0] * 129, [1.0] * 129, [0.0] * 129,
                          [0.0] * 129, [0], [0.0])
    assert err.value.code == _lib.ERR_ARG


def _problem():
    """log-uniform a, log-normal c, truncated normal b; the likelihood is
    Gaussian in log a, in log c and in b, so the evidence is a product of
    three one-dimensional integrals."""
    from nautilus_amd import Prior
    prior = Prior()
    prior.add_parameter('a', dist=stats.loguniform(1e-2, 1e2))
    prior.add_parameter('f', dist=1.5)
    prior.add_parameter('c', dist=stats.lognorm(0.7))
    prior.add_parameter('b', dist=stats.truncnorm(-1.0, 3.0, loc=1.0))
    prior.add_parameter('a2', dist='a')
    return prior


GAUSS = dict(a=(0.5, 0.3), c=(0.2, 0.25), b=(1.5, 0.3))   # (mean, width)


def _exact():
    """log Z, and the posterior mean and standard deviation of each free
    parameter, by quadrature of prior x likelihood (for a and c the evidence
    is also known in closed form and checked against it)."""
    from scipy.integrate import quad
    prior = _problem()
    dists = dict(zip(prior.keys, prior.dists))
    log_z, moments = 0.0, {}
    for key, (m, w) in GAUSS.items():
        def like(x):
            t = x if key == 'b' else np.log(x)
            return np.exp(-0.5 * ((t - m) / w)**2)
        lo, hi = dists[key].support()
        if key == 'c':
            lo, hi = np.exp(m - 12 * w), np.exp(m + 12 * w)
        peak = m if key == 'b' else np.exp(m)
        grid = [peak * f for f in (0.5, 0.8, 1.0, 1.25, 2.0)]
        mom = [quad(lambda x: x**k * dists[key].pdf(x) * like(x), lo, hi,
                    points=grid, epsabs=0, epsrel=1e-11, limit=400)[0]
               for k in range(3)]
        log_z += np.log(mom[0])
        mean = mom[1] / mom[0]
        moments[key] = (mean, np.sqrt(mom[2] / mom[0] - mean**2), mom[0])
    z_a = 0.3 * np.sqrt(2 * np.pi) / np.log(1e4)
    z_c = 0.25 * np.sqrt(2 * np.pi) * stats.norm.pdf(
        0.2, loc=0.0, scale=np.hypot(0.7, 0.25))
    assert abs(moments['a'][2] / z_a - 1) < 1e-9
    assert abs(moments['c'][2] / z_c - 1) < 1e-9
    return log_z, moments


def test_sampler_with_device_prior_families():
    """End to end: the physical points never leave the GPU, the likelihood
    receives contiguous cuda tensors, the evidence and the posterior means
    are the quadrature values, and a seed fixes the run."""
    import torch
    from nautilus_amd import Sampler

    def like(p):
        for key in 'afcb':
            assert isinstance(p[key], torch.Tensor) and p[key].is_cuda
            assert p[key].is_contiguous() and p[key].dim() == 1
        assert torch.equal(p['a2'], p['a']) and float(p['f'][0]) == 1.5
        out = 0.0
        for key, (m, w) in GAUSS.items():
            t = p[key] if key == 'b' else torch.log(p[key])
            out = out - 0.5 * ((t - m) / w)**2
        return out
    like.device = True
    log_z, moments = _exact()
    runs = []
    for _ in range(2):
        s = Sampler(_problem(), like, n_live=500, n_networks=1,
                    vectorized=True, seed=4)
        s.run(n_eff=5000, discard_exploration=True)
        runs.append(s)
    s = runs[0]
    print('log Z %.4f, exact %.4f' % (s.log_z, log_z))
    assert abs(s.log_z - log_z) < 0.05
    pts, log_w, _ = s.posterior(return_as_dict=True)
    weights = np.exp(log_w)
    for key, (mean, sd, _) in moments.items():
        got = np.average(pts[key], weights=weights)
        print('%s: mean %.5f, exact %.5f, posterior sd %.5f' % (key, got,
                                                               mean, sd))
        assert abs(got - mean) < 5 / np.sqrt(5000) * sd, key
    assert np.array_equal(pts['a2'], pts['a']) and np.all(pts['f'] == 1.5)
    # same seed, same run (test_same_seed_same_result's rule) and same points
    assert (runs[0].log_z, runs[0].n_like) == (runs[1].log_z, runs[1].n_like)
    again = runs[1].posterior(return_as_dict=True)
    for key in pts:
        assert np.array_equal(pts[key], again[0][key])
    assert np.array_equal(log_w, again[1])
