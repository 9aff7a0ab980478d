"""The device Gaussian-process likelihood of an ordered series with a sum of
kernel terms (``nb_gps_create_terms`` / ``nb_gps_loglike``,
nautilus_amd/csrc/nb_gps_filter.h) against its recursion in
``np.longdouble``, its bit-for-bit independence of the batch and of the order
of the terms, its NaN rules, the dense kernel ``nb_gp_loglike`` and the
single-term kernel on the same inputs, its C ABI, and end to end through
``Sampler``.  The problems, the truth and the tolerance (``case_budget``:
eight times the float64 twin's own error against the truth, at least 64 eps
of the value) live in test_gps_terms.py."""

import functools
import itertools

import numpy as np
import pytest

import test_gp_likelihood as dense
from nautilus_amd.likelihoods import GPS_STATES
from test_gps_likelihood import DENSE_N, LD, budget, identity, make
from test_gps_terms import (COMBOS, bad_hyper, case_budget, columns,
                            covariance, name_of, permuted, problem, truth,
                            width, without)

pytestmark = pytest.mark.gpu

N_ALL = (1, 63, 64, 65, 130)
LONG = (('sho', 'sho', 'sho'), ('matern52', 'matern52'),
        ('exp', 'matern32', 'matern52'), ('exp', 'sho'))
# the triples of six states, and one pair
SIX = tuple(c for c in COMBOS
            if len(c) == 3 and sum(GPS_STATES[k] for k in c) == 6)
BITS = SIX + (('exp', 'sho'),)


def block():
    from nautilus_amd import device
    return device.GPS_BLOCK


def _cuda(*arrays):
    import torch
    return [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in arrays]


# index of P in (1, 2, C - 1, C, C + 1, 2 C + 1); n rotates so that every n
# meets every P; and P = 600, across two renormalisations, for four
SHAPES = [(ip, N_ALL[(ip + ik) % 5], kernel)
          for ik, kernel in enumerate(COMBOS) for ip in range(6)] + \
         [(6, N_ALL[1 + ik], kernel) for ik, kernel in enumerate(LONG)]


def test_shapes():
    from nautilus_amd import device
    assert device.GPS_BLOCK >= 4 and device.GPS_BLOCK % 2 == 0
    assert len(COMBOS) == 23 and len(SIX) == 6
    assert set(LONG) <= set(COMBOS)
    for ip in range(6):
        assert {n for i, n, _ in SHAPES if i == ip} == set(N_ALL)


@pytest.mark.parametrize('ip, n, kernel', SHAPES,
                         ids=lambda v: name_of(v) if isinstance(v, tuple)
                         else str(v))
def test_values(ip, n, kernel):
    """|device - long double| <= case_budget in every row."""
    import torch
    c = block()
    p = (1, 2, c - 1, c, c + 1, 2 * c + 1, 600)[ip]
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
              p, n, name_of(kernel), (err / tol).max(), err.max(),
              (err / np.abs(want.astype(float))).max()))
    assert np.all(np.isfinite(got))
    assert np.all(err <= tol), (err / tol).max()
    # the constant joins with one subtraction: log_norm - sum / 2
    like = make(t, d, sigma, kernel, normalised=True)
    assert np.array_equal(like.from_model(mt, ht).cpu().numpy(),
                          like.log_norm + got)
    # numpy in, numpy out
    if ip == 4:
        assert np.array_equal(raw.from_model(m, h), got)


@pytest.mark.parametrize('kernel', BITS, ids=name_of)
def test_rows_bit_for_bit(kernel):
    """A row's bits are those it has alone, inside a batch of 17 and inside a
    batch of 130 at different positions, with m and h each in place inside a
    wider tensor, on any stream."""
    import torch
    n, p = 130, 2 * block() + 6
    w = width(kernel)
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
    hwide = torch.from_numpy(rng.normal(size=(n, 13))).cuda()
    hwide[:, 1:1 + w] = hbig
    hview = hwide[:, 1:1 + w]
    assert hview.data_ptr() == hwide.data_ptr() + 8
    assert hview.stride() == (13, 1)
    assert torch.equal(like.from_model(view, hbig), full)
    assert torch.equal(like.from_model(big, hview), full)
    assert torch.equal(like.from_model(view, hview), full)
    table = like._table()
    assert table.width == w
    assert torch.equal(table.loglike(view, hview, ld=p + 5, ld_hyper=13), full)
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


@pytest.mark.parametrize('kernel', COMBOS, ids=name_of)
def test_the_order_of_the_terms_changes_no_bit(kernel):
    """The names in any order with their columns (equal names in order)
    select the same kernel and give the same bits."""
    import torch
    p, n = block() + 3, 65
    t, d, sigma, m, h = problem(p, n, kernel)
    mt, ht = _cuda(m, h)
    want = make(t, d, sigma, kernel).from_model(mt, ht)
    assert bool(torch.isfinite(want).all())
    count = 0
    for perm in itertools.permutations(range(len(kernel))):
        other, h2 = permuted(kernel, h, perm)
        if other == kernel or any(
                other[i] == other[j] and perm[i] > perm[j]
                for i in range(len(perm)) for j in range(i + 1, len(perm))):
            continue
        count += 1
        got = make(t, d, sigma, other).from_model(mt, _cuda(h2)[0])
        assert torch.equal(got, want), other
    assert count == len(set(itertools.permutations(kernel))) - 1


@pytest.mark.parametrize('kernel', COMBOS, ids=name_of)
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
    causes = [('h', col, v) for col, v in bad_hyper(kernel)]
    causes += [('m', col, v) for col in (0, block() - 1, block(), p - 1)
               for v in (float('nan'), float('inf'), -float('inf'))]
    for what, col, value in causes:
        m2, h2 = mt.clone(), ht.clone()
        (h2 if what == 'h' else m2)[places, col] = value
        got = like.from_model(m2, h2)
        assert bool(torch.isnan(got[places]).all()), (what, col, value)
        assert torch.equal(got[rest], clean[rest]), (what, col, value)
    # several causes at once, one per place
    m2, h2 = mt.clone(), ht.clone()
    for i, (what, col, value) in zip(places, causes[::5]):
        (h2 if what == 'h' else m2)[i, col] = value
    got = like.from_model(m2, h2)
    assert bool(torch.isnan(got[places]).all())
    assert torch.equal(got[rest], clean[rest])
    # a_i = 0 is legal, one term at a time and all at once (white noise)
    for cols in [[c] for c in columns(kernel)] + [columns(kernel)]:
        h3 = ht.clone()
        h3[:, cols] = 0.0
        assert bool(torch.isfinite(like.from_model(mt, h3)).all())
    # equal times (problem has a pair) without any noise are unspecified for
    # a sum: those rows are NaN or finite, the others keep their bits
    bare = make(t, d, None, kernel)
    h4 = ht.clone()
    h4[places, -1] = 0.0
    got = bare.from_model(mt, h4)
    assert not bool(torch.isinf(got).any())
    assert bool(torch.isfinite(got[rest]).all())
    assert torch.equal(got[rest], bare.from_model(mt, ht)[rest])


@pytest.mark.parametrize('kernel', (('sho', 'sho'), ('exp', 'matern32'),
                                    ('sho', 'sho', 'sho')), ids=name_of)
@pytest.mark.parametrize('p', (16, 128))
def test_against_the_dense_kernel(p, kernel):
    """``nb_gps_loglike`` against ``nb_gp_loglike`` in cov='full' on the K
    built in numpy, within the sum of the two budgets.  The dense kernel's is
    ``budget`` of test_gp_likelihood.py with its term for covariance elements
    that were built in float64 from (a, l), at a = sum a_i: an element of this
    K is a sum of such elements."""
    from nautilus_amd import GaussianProcessLikelihood
    t, d, sigma, m, h = problem(p, DENSE_N, kernel)
    other = GaussianProcessLikelihood(identity, t, d, sigma, cov='full',
                                      normalised=False)
    k = covariance(kernel, other.dist, h, np.float64)
    mt, ht, kt = _cuda(m, h, k)
    got = make(t, d, sigma, kernel).from_model(mt, ht).cpu().numpy()
    want = other.from_model(mt, kt).cpu().numpy()
    ref = dense.reference(other.dist, d, sigma, m, k, 'full', None)
    tol = case_budget(p, DENSE_N, kernel) + \
        dense.budget(p, ref, h[:, columns(kernel)].sum(axis=1)).total
    err = np.abs(got - want)
    print('P = %d, %s: largest used fraction of the two budgets %.3g' % (
        p, name_of(kernel), (err / tol).max()))
    assert np.all(np.isfinite(got)) and np.all(np.isfinite(want))
    assert np.all(err <= tol), (err / tol).max()


def single_hyper(name, h2):
    """(a, l[, q], s) -> the single term's (a, l, s[, q])"""
    return h2[:, [0, 1, 3, 2]] if name == 'sho' else h2


def single_case(t, d, sigma, m, name, h1):
    """Device value, long-double truth and budget of the single-term path."""
    like = make(t, d, sigma, name)
    got = like.from_model(*_cuda(m, h1)).cpu().numpy()
    want = like.numpy_from_model(m, h1, dtype=LD)
    return got, want, budget(like.numpy_from_model(m, h1), want)


@pytest.mark.parametrize('kernel', [c for c in COMBOS if len(c) == 2],
                         ids=name_of)
def test_a_pair_with_a_zero_against_the_single_term_kernel(kernel):
    """Within the sum of the two budgets, each kernel's against its own
    long-double twin on these inputs."""
    p, n = 2 * block() + 1, 65
    t, d, sigma, m, h = problem(p, n, kernel)
    for i in range(2):
        h0 = h.copy()
        h0[:, columns(kernel)[i]] = 0.0
        like = make(t, d, sigma, kernel)
        got = like.from_model(*_cuda(m, h0)).cpu().numpy()
        mine = like.numpy_from_model(m, h0, dtype=LD)
        tol = budget(like.numpy_from_model(m, h0), mine)
        (name,), h2 = without(kernel, h0, i)
        other, _, tol_other = single_case(t, d, sigma, m, name,
                                          single_hyper(name, h2))
        err = np.abs(got - other)
        print('%s without term %d: largest used fraction of the two budgets '
              '%.3g' % (name_of(kernel), i, (err / (tol + tol_other)).max()))
        assert np.all(np.isfinite(got)) and np.all(np.isfinite(other))
        assert np.all(err <= tol + tol_other)


def test_two_halves_of_an_exponential_against_the_single_term_kernel():
    p, n = 2 * block() + 1, 65
    kernel = ('exp', 'exp')
    t, d, sigma, m, h = problem(p, n, kernel)
    h2 = h.copy()
    h2[:, 0] = h2[:, 2] = 0.5 * h[:, 0]
    h2[:, 3] = h[:, 1]
    like = make(t, d, sigma, kernel)
    got = like.from_model(*_cuda(m, h2)).cpu().numpy()
    mine = like.numpy_from_model(m, h2, dtype=LD)
    tol = budget(like.numpy_from_model(m, h2), mine)
    other, _, tol_other = single_case(t, d, sigma, m, 'exp', h[:, [0, 1, 4]])
    err = np.abs(got - other)
    print('exp as two halves: largest used fraction of the two budgets %.3g' %
          (err / (tol + tol_other)).max())
    assert np.all(np.isfinite(got)) and np.all(err <= tol + tol_other)


def test_a_triple_with_a_zero_has_the_bits_of_the_pair():
    """On the device as in the twin: the switched-off block stays zero and
    adds zeros."""
    import torch
    p, n = block() + 3, 65
    for kernel in (('exp', 'matern32', 'matern52'), ('sho', 'sho', 'sho'),
                   ('exp', 'exp', 'sho')):
        t, d, sigma, m, h = problem(p, n, kernel)
        for i in range(3):
            h0 = h.copy()
            h0[:, columns(kernel)[i]] = 0.0
            got = make(t, d, sigma, kernel).from_model(*_cuda(m, h0))
            other, h2 = without(kernel, h0, i)
            want = make(t, d, sigma, other).from_model(*_cuda(m, h2))
            assert bool(torch.isfinite(want).all())
            assert torch.equal(got, want), (kernel, i)


def test_argument_errors_carry_err_arg():
    import ctypes
    import torch
    from nautilus_amd import _lib, device

    t = np.array([0.0, 1.0, 1.0])
    d = np.array([0.5, -2.0, 5.5])
    assert device.GPSTable(t, d, kernel=('exp', 'sho')).width == 6
    assert device.GPSTable(t, d, np.r_[0.0, 1.0, 4.0],
                           kernel=['sho', 'sho', 'sho'],
                           log_norm=-3.0).width == 10
    for kernel in (('exp',), ('exp',) * 4, ('matern52', 'matern52', 'exp')):
        with pytest.raises(_lib.NativeError) as err:
            device.GPSTable(t, d, kernel=kernel)
        assert err.value.code == _lib.ERR_ARG
        assert 'Gaussian-process series likelihood' in str(err.value)
    # pack_gps's own refusals come through with their messages
    with pytest.raises(_lib.NativeError, match='t must not decrease'):
        device.GPSTable(np.r_[0.0, 2.0, 1.0], d, kernel=('exp', 'sho'))
    with pytest.raises(_lib.NativeError, match='sigma2 1 must be finite'):
        device.GPSTable(t, d, np.r_[0.0, -1.0, 1.0], kernel=('exp', 'sho'))
    with pytest.raises(ValueError, match='kernel must be one of'):
        device.GPSTable(t, d, kernel=('exp', 'sqexp'))
    lib = _lib.load()
    h = ctypes.c_void_p()

    def raw_refused(text, fn, *args):
        # another entry's message first: the text checked below is this call's
        assert lib.nb_poisson_create(0, None, None, None, 0.0,
                                     None) == _lib.ERR_ARG
        assert b'Poisson' in lib.nb_last_error()
        assert fn(*args) == _lib.ERR_ARG
        message = lib.nb_last_error()
        assert b'Gaussian-process series likelihood' in message
        assert text in message, message

    tp = t.ctypes.data_as(_lib.c_double_p)
    dp = d.ctypes.data_as(_lib.c_double_p)

    def codes(*values):
        arr = np.array(values, dtype=np.int32)
        return arr.ctypes.data_as(_lib.c_int32_p), arr

    two, keep = codes(0, 3)
    create = lib.nb_gps_create_terms
    raw_refused(b'no NULL pointer', create, 3, None, dp, None, 2, two, 0.0,
                ctypes.byref(h))
    raw_refused(b'no NULL pointer', create, 3, tp, None, None, 2, two, 0.0,
                ctypes.byref(h))
    raw_refused(b'no NULL pointer', create, 3, tp, dp, None, 2, None, 0.0,
                ctypes.byref(h))
    raw_refused(b'no NULL pointer', create, 3, tp, dp, None, 2, two, 0.0, None)
    for count in (0, 1, 4, -1):
        ptr, keep4 = codes(0, 0, 0, 0)
        raw_refused(b'2..3 terms, not %d' % count, create, 3, tp, dp, None,
                    count, ptr, 0.0, ctypes.byref(h))
    ptr, keep2 = codes(0, 4)
    raw_refused(b'term 1 of', create, 3, tp, dp, None, 2, ptr, 0.0,
                ctypes.byref(h))
    ptr, keep3 = codes(-1, 0, 0)
    raw_refused(b'term 0 of', create, 3, tp, dp, None, 3, ptr, 0.0,
                ctypes.byref(h))
    ptr, keep5 = codes(2, 2, 0)
    raw_refused(b'7 states', create, 3, tp, dp, None, 3, ptr, 0.0,
                ctypes.byref(h))
    raw_refused(b'n_data', create, 0, tp, dp, None, 2, two, 0.0,
                ctypes.byref(h))
    raw_refused(b'log_norm', create, 3, tp, dp, None, 2, two, float('nan'),
                ctypes.byref(h))
    assert not h.value
    # a single-term handle is still refused at kernel code 4
    raw_refused(b'NB_GPS_EXP .. NB_GPS_SHO', lib.nb_gps_create, 3, tp, dp,
                None, 4, 0.0, ctypes.byref(h))

    pair = device.GPSTable(t, d, np.ones(3), kernel=('exp', 'sho'))
    one = device.GPSTable(t, d, np.ones(3), kernel='sho')
    m = torch.ones(4, 3, dtype=torch.float64, device='cuda')
    h6 = torch.ones(4, 6, dtype=torch.float64, device='cuda')
    h4 = torch.ones(4, 4, dtype=torch.float64, device='cuda')

    def refused(tab, *args, **kw):
        with pytest.raises(_lib.NativeError) as err:
            tab.loglike(*args, **kw)
        assert err.value.code == _lib.ERR_ARG
        assert 'Gaussian-process series likelihood' in str(err.value)
        return str(err.value)

    # the width follows the handle
    assert 'ld_hyper >= 6' in refused(pair, m, h6, ld_hyper=5)
    assert 'ld_hyper >= 6' in refused(pair, m, h6, ld=2)
    assert 'ld_hyper >= 4' in refused(one, m, h4, ld_hyper=3)
    want = pair.loglike(m, h6)
    assert want.shape == (4,) and bool(torch.isfinite(want).all())
    assert torch.equal(pair.loglike(m, h6, ld=3, ld_hyper=6), want)
    assert torch.equal(pair.loglike(m[:1], h6[:1], ld=0, ld_hyper=0),
                       want[:1])
    out = torch.empty(4, dtype=torch.float64, device='cuda')
    ptrs = dict(m=m.data_ptr(), c=h6.data_ptr(), out=out.data_ptr())
    for null in ('m', 'c', 'out'):
        a = dict(ptrs)
        a[null] = None
        raw_refused(b'no NULL pointer', lib.nb_gps_loglike, pair._h, a['m'],
                    3, a['c'], 6, 4, a['out'], None)
    assert lib.nb_gps_loglike(pair._h, None, 3, None, 6, 0, None, None) == 0
    with pytest.raises(ValueError):
        pair.loglike(m, h6[:3])


# ---------------------------------------------------------- through Sampler

SERIES_TRUE = (0.7, 1.0, 10.0, 0.3, 0.2)      # mean, a1, l1, a2, l2
SERIES_S = 1e-4                               # held fixed by the model
SERIES_SIGMA = 0.05
SERIES_P = 1024
SERIES_SEED = 2028


@functools.lru_cache(maxsize=None)
def _series(seed=SERIES_SEED):
    """1024 samples of a Matern-3/2 plus an exponential process with a
    constant mean at sorted uniform times in [0, 300], error bars of 0.05,
    drawn once."""
    from nautilus_amd.likelihoods import gp_correlation
    rng = np.random.default_rng(seed)
    t = np.sort(rng.uniform(0, 300, size=SERIES_P))
    mean, a1, l1, a2, l2 = SERIES_TRUE
    dist = np.abs(t[:, None] - t[None, :])
    k = a1 * gp_correlation('matern32', dist / l1) + \
        a2 * gp_correlation('exp', dist / l2) + \
        (SERIES_S + SERIES_SIGMA**2) * np.eye(SERIES_P)
    return t, mean + np.linalg.cholesky(k) @ rng.normal(size=SERIES_P)


def sample_series(seed=SERIES_SEED):
    import torch
    from scipy import stats
    from nautilus_amd import GaussianProcessSeriesLikelihood, Prior, Sampler
    t, data = _series(seed)

    def model(x):
        s = torch.full((x.shape[0], 1), SERIES_S, dtype=x.dtype,
                       device=x.device)
        return (x[:, :1].expand(x.shape[0], SERIES_P),
                torch.cat([x[:, 1:], s], dim=1))

    like = GaussianProcessSeriesLikelihood(
        model, t, data, np.full(SERIES_P, SERIES_SIGMA),
        kernel=('matern32', 'exp'))
    prior = Prior()
    prior.add_parameter('mean', dist=stats.uniform(-3.0, 6.0))
    for name, (lo, hi) in zip(('a1', 'l1', 'a2', 'l2'),
                              ((0.05, 20.0), (1.0, 100.0), (0.01, 5.0),
                               (0.01, 1.0))):
        prior.add_parameter(name, dist=stats.loguniform(lo, hi))
    assert prior.device                      # transformed on the GPU
    s = Sampler(prior, like, pass_dict=False, n_live=400, vectorized=True,
                seed=0)
    s.run(n_eff=2000, discard_exploration=True)
    return s


def z_scores(s):
    pts, log_w, _ = s.posterior()
    wgt = np.exp(log_w - np.max(log_w))
    x = np.concatenate([pts[:, :1], np.log(pts[:, 1:])], axis=1)
    mean = wgt @ x / wgt.sum()
    sd = np.sqrt(wgt @ (x - mean)**2 / wgt.sum())
    want = np.r_[SERIES_TRUE[0], np.log(SERIES_TRUE[1:])]
    return (mean - want) / sd, sd


def test_sampler_recovers_the_hyper_parameters_of_two_terms():
    """Mean and log a, log l of both terms of a simulated series through
    ``Sampler`` with a device prior, s held fixed by the model: every truth
    within four posterior standard deviations of the posterior mean, and the
    run repeats bit for bit."""
    s = sample_series()
    z, sd = z_scores(s)
    print('log Z = %.3f, n_like = %d, n_eff = %.0f; (mean - truth) / sd:' % (
        s.log_z, s.n_like, s.n_eff), z, 'sd', sd)
    assert np.all(np.isfinite(z)) and np.all(sd > 0)
    assert np.all(np.abs(z) < 4)
    again = sample_series()
    assert again.log_z == s.log_z and again.n_like == s.n_like
