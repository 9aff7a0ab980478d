"""The fused device Poisson likelihood of binned counts
(``nb_poisson_loglike``, nautilus_amd/csrc/nb_poisson.hip) against its numpy
twin under a derived error bound, its bit-for-bit independence of the batch,
its edge-case rules, and end to end through ``Sampler``."""

import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

EPS = 2.0**-52

# every P and every n of the two lists appears; the kernel changes its shape
# after P = 32 and after P = 512
P_ALL = (1, 3, 15, 16, 17, 63, 64, 65, 257, 1025, 4099)
N_ALL = (1, 15, 17, 1000, 4097)
# (P, n, rot): a column's class is (j + rot) % 6, see problem().  From P = 6
# on a case holds every class; P = 1 and P = 3 cannot, and run once per rot
# instead, so that every class meets them too.
SHAPES = [(p, N_ALL[(i + s) % 5], 0) for i, p in enumerate(P_ALL[2:])
          for s in (0, 2)] + \
    [(p, N_ALL[(rot + p) % 5], rot) for p in (1, 3) for rot in range(6)]
assert {s[0] for s in SHAPES} == set(P_ALL)
assert {s[1] for s in SHAPES} == set(N_ALL)


def identity(x):
    return x


@functools.lru_cache(maxsize=None)
def problem(p, n, rot=0):
    """Counts, exposure, background and n model rows.  Column j is of class
    (j + rot) % 6:
      0  k = 0;
      1  k ~ Poisson(20) + 1 with a power of two as exposure and a multiple
         of 1/4 as background, so that every seventh row can hold mu = k
         exactly;
      2  k ~ Poisson(1e7);
      3  mu / k ~ 1e-12 (no background);
      4  mu / k ~ 1e12;
      5  k ~ Poisson(20), like every class without a ratio of its own at
         mu / k = exp(s N(0, 1)), s cycling over 1e-6, 1e-3, 0.1, 1, 3 with
         the row.
    Computed once per shape; nobody writes to it."""
    rng = np.random.default_rng(100000 * rot + 1000 * p + n)
    cls = (np.arange(p) + rot) % 6
    k = rng.poisson(20.0, size=p).astype(float)
    k[cls == 0] = 0.0
    k[cls == 1] += 1.0
    k[cls == 2] = rng.poisson(1e7, size=p)[cls == 2]
    e = 0.5 + rng.random(p)
    e[cls == 1] = np.where(np.arange(p) % 4 < 2, 0.5, 2.0)[cls == 1]
    b = 0.25 * (np.arange(p) % 4) * (1.0 + (cls != 1) * rng.random(p))
    b[cls == 3] = 0.0
    spread = np.array([1e-6, 1e-3, 0.1, 1.0, 3.0])[np.arange(n) % 5][:, None]
    ratio = np.exp(spread * rng.normal(size=(n, p)))
    ratio[:, cls == 3] = 1e-12 * (1 + 0.1 * rng.random((n, p)))[:, cls == 3]
    ratio[:, cls == 4] = 1e12 * (1 + 0.1 * rng.random((n, p)))[:, cls == 4]
    m = k * ratio / e
    m[:, cls == 0] = (3.0 * rng.exponential(size=(n, p)) / e)[:, cls == 0]
    exact = (np.arange(n) % 7 == 0)[:, None] & (cls == 1)
    m = np.where(exact, (k - b) / e, m)
    for arr in (k, e, b, m):
        arr.setflags(write=False)
    return k, e, b, m


def budget(k, e, b, m, d):
    """eps (8 sum_j B_ij + P sum_j D_ij), B = |mu - k| + k |log(mu / k)| (mu
    for k = 0): per element one subtraction, two multiplications, a log or
    log1p at <= 2 ulp, one subtraction and one multiplication, and the error
    of mu itself through |1 - k / mu| mu <= B; summing P non-negative terms
    in any order costs at most P eps of the sum."""
    mu = e * m + b
    with np.errstate(divide='ignore', invalid='ignore'):
        lg = np.where(k > 0, np.log(mu / np.where(k > 0, k, 1.0)), 0.0)
    big = np.where(k > 0, np.abs(mu - k) + k * np.abs(lg), mu)
    return EPS * (8 * big.sum(1) + len(k) * d.sum(1))


@pytest.mark.parametrize('p, n, rot', SHAPES)
def test_values(p, n, rot):
    import torch
    from nautilus_amd import PoissonDataLikelihood
    k, e, b, m = problem(p, n, rot)
    cls = (np.arange(p) + rot) % 6
    mu = e * m + b
    # what the case holds, checked on the host
    assert np.all(np.isfinite(mu)) and np.all(mu > 0)
    t = (mu - k)[:, k > 0] / k[k > 0]
    for c, have in ((0, np.any(k == 0)), (1, np.any(mu == k)),
                    (2, np.any(k > 5e6)),
                    (3, t.size and np.any(np.abs(1 + t) < 2e-12)),
                    (4, t.size and np.any(t > 5e11))):
        assert bool(have) == bool(np.any(cls == c)), c
    assert np.any(e != 1.0)
    if p >= 6:
        assert np.all(np.isin(np.arange(6), cls)) and np.any(b != 0.0)
        # both log branches
        assert np.any(np.abs(t) < 0.5) and np.any(np.abs(t) >= 0.5)
    raw = PoissonDataLikelihood(identity, k, exposure=e, background=b,
                                normalised=False)
    d = raw.numpy_deviance(m)
    twin = raw.numpy_from_model(m)
    assert np.all(np.isfinite(twin))
    tol = budget(k, e, b, m, d)
    mt = torch.from_numpy(m).cuda()
    out = raw.from_model(mt)
    assert out.is_cuda and out.dtype == torch.float64 and out.shape == (n,)
    got = out.cpu().numpy()
    used = np.abs(got - twin) / np.where(tol > 0, tol, 1.0)
    print('P = %d, n = %d, rot = %d: largest used fraction of the bound %.3g'
          % (p, n, rot, used.max()))
    assert np.all(np.isfinite(got))
    assert np.all(np.abs(got - twin) <= tol), used.max()
    # the constant joins with one subtraction: log_const - sum, bit for bit
    like = PoissonDataLikelihood(identity, k, exposure=e, background=b)
    assert like.log_const != 0.0 or np.all(k <= 1)
    assert np.array_equal(like.from_model(mt).cpu().numpy(),
                          like.log_const - (-got))


def test_both_log_branches_are_exercised():
    small = big = 0
    for p, n, rot in SHAPES:
        k, e, b, m = problem(p, n, rot)
        t = ((e * m + b) - k)[:, k > 0] / k[k > 0]
        small += int(np.sum(np.abs(t) < 0.5))
        big += int(np.sum(np.abs(t) >= 0.5))
    print('|t| < 1/2: %d elements, |t| >= 1/2: %d' % (small, big))
    assert small > 1000 and big > 1000


@pytest.mark.parametrize('p', [3, 129, 1025])
def test_rows_bit_for_bit(p):
    """A row's bits are those it has alone, inside batches of 17 and 4097 at
    different positions, with ld = P and ld = P + 5, on any stream."""
    import torch
    from nautilus_amd import PoissonDataLikelihood
    k, e, b, m = problem(p, 4097)
    like = PoissonDataLikelihood(identity, k, exposure=e, background=b)
    big = torch.from_numpy(m).cuda()
    full = like.from_model(big)
    assert bool(torch.isfinite(full).all())
    for off in (0, 1, 777, 4080):
        sub = big[off:off + 17]
        assert sub.data_ptr() == big.data_ptr() + off * p * 8   # a view
        assert torch.equal(like.from_model(sub), full[off:off + 17]), off
        for r in (off, off + 16):
            assert torch.equal(like.from_model(big[r:r + 1]), full[r:r + 1])
    # the same rows at other positions of a batch
    perm = torch.from_numpy(np.random.default_rng(p).permutation(4097)).cuda()
    assert torch.equal(like.from_model(big[perm]), full[perm])
    assert like.from_model(big[:0]).shape == (0,)
    # a column slice of a wider tensor: rows P + 5 doubles apart
    wide = torch.from_numpy(
        np.random.default_rng(p).normal(size=(4097, p + 5))).cuda()
    wide[:, 2:2 + p] = big
    view = wide[:, 2:2 + p]
    assert view.data_ptr() == wide.data_ptr() + 2 * 8
    assert view.stride() == (p + 5, 1)
    assert torch.equal(like.from_model(view), full)
    table = like._table()
    assert torch.equal(table.loglike(view, ld=p + 5), full)
    assert torch.equal(table.loglike(view[5:22]), full[5:22])
    assert torch.equal(table.loglike(view[40:41]), full[40:41])
    # a stream of its own
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        other = like.from_model(big)
        one = like.from_model(view[9:10])
    stream.synchronize()
    assert torch.equal(other, full) and torch.equal(one, full[9:10])


@pytest.mark.parametrize('p', [17, 129, 1025])
def test_edge_rows(p):
    import torch
    from nautilus_amd import PoissonDataLikelihood
    k, e, b, m = problem(p, 1000)
    like = PoissonDataLikelihood(identity, k, exposure=e, background=b)
    clean = torch.from_numpy(m[:100].copy()).cuda()
    want = like.from_model(clean)
    assert bool(torch.isfinite(want).all())
    cls = np.arange(p) % 6
    c_zero = int(np.flatnonzero(cls == 0)[-1])         # k = 0
    c_dead = int(np.flatnonzero(cls == 3)[0])          # k > 0, no background
    c_last = p - 1
    assert k[c_zero] == 0 and k[c_dead] > 0 and b[c_dead] == 0
    dirty = clean.clone()
    dirty[3, c_dead] = 0.0                             # mu = 0, k > 0
    dirty[11, c_last] = -1e300                         # negative
    dirty[12, c_zero] = -(b[c_zero] + 1.0) / e[c_zero]     # negative, k = 0
    dirty[40, 0] = float('nan')
    dirty[41, c_last] = float('inf')
    dirty[42, 1] = float('-inf')
    dirty[77, c_dead] = 0.0                            # -inf and NaN together
    dirty[77, c_last] = float('nan')
    dirty[99, c_dead] = 0.0
    dirty[99, c_zero] = float('inf')
    out = like.from_model(dirty)
    assert float(out[3]) == -np.inf
    for i in (11, 12, 40, 41, 42, 77, 99):
        assert bool(torch.isnan(out[i])), i
    keep = torch.ones(100, dtype=torch.bool, device='cuda')
    keep[[3, 11, 12, 40, 41, 42, 77, 99]] = False
    assert torch.equal(out[keep], want[keep])
    twin = like.numpy_from_model(dirty.cpu().numpy())
    assert np.array_equal(np.isnan(twin), torch.isnan(out).cpu().numpy())
    assert np.array_equal(np.isneginf(twin), torch.isinf(out).cpu().numpy())
    # mu = 0 where k = 0 contributes nothing: a finite row
    raw = PoissonDataLikelihood(identity, k, exposure=e, normalised=False)
    row = clean[5:6].clone()
    row[0, c_zero] = 0.0
    got = float(raw.from_model(row)[0])
    twin = raw.numpy_from_model(row.cpu().numpy())[0]
    d = raw.numpy_deviance(row.cpu().numpy())
    assert d[0, c_zero] == 0.0 and np.isfinite(got)
    assert abs(got - twin) <= budget(k, e, 0 * b, row.cpu().numpy(), d)[0]


def test_one_handle_on_two_streams():
    import torch
    from nautilus_amd import PoissonDataLikelihood
    k, e, b, m = problem(257, 1000)
    like = PoissonDataLikelihood(identity, k, exposure=e, background=b)
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
            device.PoissonTable(*args, **kw)
        assert str(err.value)
        return err.value.code

    k = np.array([0.0, 2.0, 5.5])
    one = np.ones(3)
    assert device.PoissonTable(k).n_data == 3
    assert device.PoissonTable(k, one, 0 * one, log_const=-3.0).n_data == 3
    # n_data outside 1 .. 2^20
    assert code(np.zeros(0)) == _lib.ERR_ARG
    assert code(np.zeros((1 << 20) + 1)) == _lib.ERR_ARG
    assert device.PoissonTable(np.zeros(1 << 20)).n_data == 1 << 20
    # counts
    assert code(np.r_[1.0, np.nan, 1.0]) == _lib.ERR_ARG
    assert code(np.r_[1.0, np.inf, 1.0]) == _lib.ERR_ARG
    assert code(np.r_[1.0, -0.5, 1.0]) == _lib.ERR_ARG
    assert code(np.r_[1.0, 1e-310, 1.0]) == _lib.ERR_ARG    # 1 / k = inf
    # exposure, background, constant
    for bad in (0.0, -1.0, np.nan, np.inf):
        assert code(k, exposure=np.r_[1.0, bad, 1.0]) == _lib.ERR_ARG
    for bad in (-1e-9, np.nan, np.inf):
        assert code(k, background=np.r_[0.0, bad, 0.0]) == _lib.ERR_ARG
    assert code(k, log_const=np.nan) == _lib.ERR_ARG
    assert code(k, log_const=-np.inf) == _lib.ERR_ARG
    # NULL counts, NULL out
    lib = _lib.load()
    h = ctypes.c_void_p()
    assert lib.nb_poisson_create(3, None, None, None, 0.0,
                                 ctypes.byref(h)) == _lib.ERR_ARG
    assert lib.nb_poisson_create(
        3, k.ctypes.data_as(_lib.c_double_p), None, None, 0.0,
        None) == _lib.ERR_ARG
    # ld < n_data counts from the second row on
    table = device.PoissonTable(k)
    m = torch.ones(4, 3, dtype=torch.float64, device='cuda')
    with pytest.raises(_lib.NativeError) as err:
        table.loglike(m, ld=2)
    assert err.value.code == _lib.ERR_ARG and str(err.value)
    assert table.loglike(m, ld=3).shape == (4,)
    assert torch.equal(table.loglike(m[:1], ld=0), table.loglike(m)[:1])
    # NULL pointers with n > 0, and none needed for n = 0
    out = torch.empty(4, dtype=torch.float64, device='cuda')
    assert lib.nb_poisson_loglike(table._h, None, 3, 4, out.data_ptr(),
                                  None) == _lib.ERR_ARG
    assert lib.nb_poisson_loglike(table._h, m.data_ptr(), 3, 4, None,
                                  None) == _lib.ERR_ARG
    assert lib.nb_poisson_loglike(None, m.data_ptr(), 3, 4, out.data_ptr(),
                                  None) == _lib.ERR_ARG
    assert lib.nb_poisson_loglike(table._h, m.data_ptr(), 3, -1,
                                  out.data_ptr(), None) == _lib.ERR_ARG
    assert lib.nb_poisson_loglike(table._h, None, 3, 0, None, None) == 0
    assert lib.nb_poisson_destroy(None) == 0
    # shapes that do not fit together never reach the library
    with pytest.raises(ValueError):
        device.PoissonTable(k, exposure=np.ones(4))
    with pytest.raises(ValueError):
        device.PoissonTable(k, background=np.zeros(2))
    with pytest.raises(ValueError):
        device.PoissonTable(k.reshape(3, 1))


def test_from_model_layout_rules():
    import torch
    from nautilus_amd import PoissonDataLikelihood
    k, e, b, m = problem(17, 1000)
    like = PoissonDataLikelihood(identity, k, exposure=e, background=b)
    mt = torch.from_numpy(m).cuda()
    with pytest.raises(ValueError):
        like.from_model(mt[:, :16])
    with pytest.raises(ValueError):
        like.from_model(mt[0])
    with pytest.raises(ValueError):
        like.from_model(mt.float())
    want = like.from_model(mt)
    # anything but unit-stride rows is copied, and gives the same bits
    turned = mt.t().contiguous().t()
    assert turned.stride() == (1, 1000)
    assert torch.equal(like.from_model(turned), want)
    twice = torch.stack([mt, mt], dim=2)[:, :, 0]       # stride(1) == 2
    assert twice.stride(1) == 2
    assert torch.equal(like.from_model(twice), want)
    raw = PoissonDataLikelihood(identity, k, exposure=e, background=b,
                                normalised=False)
    got = raw.from_model(turned).cpu().numpy()
    tol = budget(k, e, b, m, raw.numpy_deviance(m))
    assert np.all(np.abs(got - raw.numpy_from_model(m)) <= tol)
    # numpy in, numpy out
    out = like.from_model(m)
    assert isinstance(out, np.ndarray) and out.dtype == np.float64
    assert np.array_equal(out, want.cpu().numpy())
    called = like(m)                                    # the identity model
    assert isinstance(called, np.ndarray)
    assert np.array_equal(called, out)
    assert like(mt).is_cuda and torch.equal(like(mt), want)


THETA_MAX = 150.0


@functools.lru_cache(maxsize=None)
def _rates_problem():
    """Three rates, each seen by a group of eight bins with exposures between
    1/2 and 3/2: counts drawn once from the rates (5, 20, 80)."""
    rng = np.random.default_rng(2026)
    group = np.repeat(np.arange(3), 8)
    e = 0.5 + rng.random(24)
    k = rng.poisson(np.array([5.0, 20.0, 80.0])[group] * e).astype(float)
    return group, e, k


def _run_rates():
    import torch
    from scipy import stats
    from nautilus_amd import PoissonDataLikelihood, Prior, Sampler
    group, e, k = _rates_problem()
    group_dev = torch.from_numpy(group).cuda()
    prior = Prior()
    for name in 'abc':
        prior.add_parameter(name, dist=stats.uniform(0.0, THETA_MAX))
    assert prior.device                  # transformed on the GPU
    like = PoissonDataLikelihood(lambda x: x[:, group_dev], k, exposure=e)
    s = Sampler(prior, like, pass_dict=False, n_live=1000, n_networks=2,
                vectorized=True, seed=0)
    s.run(n_eff=5000, discard_exploration=True)
    return like, s


def test_sampler_recovers_rates():
    """Evidence and posterior means in the settings and the evidence band of
    test_sampler_recovers_linear_model (test_data_likelihood_gpu.py): each
    rate's posterior is Gamma(K_g + 1, E_g) cut at theta_max, K_g and E_g the
    group's summed counts and exposures."""
    from scipy.special import gammainc, gammaln
    group, e, k = _rates_problem()
    like, s = _run_rates()
    analytic, mean, sd = 0.0, np.empty(3), np.empty(3)
    for g in range(3):
        kg, eg = k[group == g], e[group == g]
        big_k, big_e = kg.sum(), eg.sum()
        analytic += np.sum(kg * np.log(eg) - gammaln(kg + 1)) + \
            gammaln(big_k + 1) + np.log(gammainc(big_k + 1,
                                                 big_e * THETA_MAX)) - \
            (big_k + 1) * np.log(big_e) - np.log(THETA_MAX)
        mean[g] = (big_k + 1) / big_e
        sd[g] = np.sqrt(big_k + 1) / big_e
    print('log Z = %.4f, analytic %.4f, n_like = %d, n_eff = %.0f' % (
        s.log_z, analytic, s.n_like, s.n_eff))
    assert abs(s.log_z - analytic) < 0.06
    pts, log_w, _ = s.posterior()
    wgt = np.exp(log_w - np.max(log_w))
    got = wgt @ pts / wgt.sum()
    tol = 4 * sd / np.sqrt(s.n_eff)
    print('posterior mean - Gamma mean in units of the tolerance:',
          (got - mean) / tol)
    assert np.all(np.abs(got - mean) < tol)
    _, again = _run_rates()
    assert again.log_z == s.log_z and again.n_like == s.n_like
