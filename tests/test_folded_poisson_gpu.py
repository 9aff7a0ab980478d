"""The fused device Poisson likelihood behind a response matrix
(``nb_fold_poisson_loglike``, nautilus_amd/csrc/nb_fold.hip) against its
numpy twin under a derived error bound, against the unfolded kernel with an
identity response, its bit-for-bit independence of the batch, its edge-case
rules, its argument errors, and end to end through ``Sampler``."""

import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

EPS = 2.0**-52

# Every P, K and n of the three lists appears.  P: the 16-bin tile, the
# 256-bin panel and two panels; K: the 4-column MFMA step, the 16-column
# k-tile and several of them; n: the 16-point tile, the blocks of 32 and 64
# points (TPW = 2 and 4) and 16 384 = 256 * 64, from which TPW = 4 is launched.
P_ALL = (1, 15, 16, 17, 255, 257, 513, 4099)
K_ALL = (1, 3, 4, 5, 15, 16, 17, 33, 130)
N_ALL = (1, 15, 17, 31, 33, 63, 65, 1000, 16383, 16385)
# (P, K, n, rot): a bin's class is (j + rot) % 6, see problem()
SHAPES = [
    (15, 1, 17, 0), (16, 3, 1, 0), (17, 4, 15, 0), (255, 5, 63, 0),
    (257, 15, 65, 0), (513, 16, 1000, 0), (4099, 17, 33, 0),
    (257, 33, 31, 0), (513, 130, 65, 0), (17, 17, 1000, 0),
    (4099, 130, 17, 0), (255, 16, 16383, 0), (17, 5, 16385, 0),
    (257, 33, 16385, 0),
] + [(1, (1, 3, 4, 5, 16, 33)[rot], N_ALL[rot], rot) for rot in range(6)]
assert {s[0] for s in SHAPES} == set(P_ALL)
assert {s[1] for s in SHAPES} == set(K_ALL)
assert {s[2] for s in SHAPES} == set(N_ALL)


def identity(x):
    return x


@functools.lru_cache(maxsize=None)
def problem(p, ks, n, rot=0, eye=False):
    """Counts, response, exposure, background and n source rows.  R >= 0 with
    about a third exact zeros; from P = 8 on every bin j = 7 (mod 11) has a
    whole zero row (its mu is its background, which is positive), from K = 4
    on every source column c = 3 (mod 5) a whole zero column; ``eye`` makes
    R the identity instead.  s > 0, each row scattered about s = 1 by
    exp(spread N(0, 1)), spread cycling over 1e-6, 1e-3, 0.1, 1, 3 with the
    row.  With mu0 the expected counts at s = 1, bin j is of class
    (j + rot) % 6, the idea of problem() in test_poisson_likelihood_gpu.py:
      0  k = 0;
      1  k = mu0 exactly (mu = k to rounding in the rows of small spread);
      2  k ~ Poisson(1e7), the exposure scaled so that mu0 ~ 1e7;
      3  k = 1e12 mu0:  mu / k ~ 1e-12;
      4  k = 1e-12 mu0:  mu / k ~ 1e12;
      5  k ~ Poisson(20), the exposure scaled so that mu0 ~ 20.
    Computed once per shape; nobody writes to it."""
    rng = np.random.default_rng(
        1000003 * rot + 10007 * p + 101 * ks + n + 7 * eye)
    cls = (np.arange(p) + rot) % 6
    if eye:
        assert p == ks
        resp = np.eye(p)
    else:
        resp = rng.random((p, ks)) * (rng.random((p, ks)) < 0.67)
        resp[np.arange(p), np.arange(p) % ks] += 0.25
        if ks >= 4:
            resp[:, 3::5] = 0.0
        if p >= 8:
            resp[7::11] = 0.0
    e = 0.5 + rng.random(p)
    b = 0.25 * (1 + np.arange(p) % 4) * (0.5 + rng.random(p))
    fold0 = resp.sum(1)                            # the fold of s = 1
    live = fold0 > 0
    for c, level in ((2, 1e7), (5, 20.0)):
        at = (cls == c) & live
        e[at] = level / fold0[at]
    mu0 = e * fold0 + b
    k = mu0.copy()
    k[cls == 0] = 0.0
    k[cls == 2] = rng.poisson(1e7, size=p)[cls == 2]
    k[cls == 3] *= 1e12
    k[cls == 4] *= 1e-12
    k[cls == 5] = rng.poisson(20.0, size=p)[cls == 5]
    spread = np.array([1e-6, 1e-3, 0.1, 1.0, 3.0])[np.arange(n) % 5][:, None]
    s = np.exp(spread * rng.normal(size=(n, ks)))
    for arr in (k, resp, e, b, s):
        arr.setflags(write=False)
    return k, resp, e, b, s


def budget(k, resp, e, b, s, d, fold_errors):
    """The bound on |kernel - twin| per row, three parts.

    (1) budget() of test_poisson_likelihood_gpu.py for the given mu:
        eps (8 sum_j B_ij + P sum_j D_ij),  B = |mu - k| + k |log(mu / k)|
        (mu for k = 0): per element one subtraction, two multiplications, a
        log or log1p at <= 2 ulp, one subtraction and one multiplication, the
        rounding of mu = e acc + b through |1 - k / mu| mu <= B, and P eps of
        the sum for adding P non-negative terms in any order.
    (2) The dot product.  A sum of K products in float64, in any order, fused
        or not, errs by at most K eps sum_k |R_jk| |s_ik|; with the product by
        e and the sum with b,  |delta mu_ij| <= (K + 3) eps A_ij,
        A_ij = e_j sum_k |R_jk| |s_ik| + b_j.  dD / dmu = 1 - k / mu (1 for
        k = 0), so to first order D moves by |1 - k_j / mu_ij| |delta mu_ij|.
    (3) The second order of (2): d2D / dmu2 = k / mu^2, so at most
        k_j (|delta mu_ij| / mu_ij)^2, which is k_j ((K + 3) eps)^2 where
        A = mu (R >= 0, s > 0) and carries (A / mu)^2 otherwise.
    ``fold_errors`` counts (2): the kernel's dot product against a reference
    mu formed in np.longdouble is 1; against the float64 twin, whose own
    ``s @ R.T`` errs by as much, it is 2."""
    ks = resp.shape[1]
    mu = e * (s @ resp.T) + b
    amp = e * (np.abs(s) @ np.abs(resp).T) + b
    with np.errstate(divide='ignore', invalid='ignore'):
        lg = np.where(k > 0, np.log(mu / np.where(k > 0, k, 1.0)), 0.0)
        slope = np.where(k > 0, np.abs(1.0 - k / mu), 1.0)
        delta = fold_errors * (ks + 3) * EPS * amp
        second = np.where(k > 0, k * (delta / mu)**2, 0.0)   # D = mu at k = 0
    big = np.where(k > 0, np.abs(mu - k) + k * np.abs(lg), mu)
    return EPS * (8 * big.sum(1) + len(k) * d.sum(1)) + \
        (slope * delta).sum(1) + second.sum(1)


@pytest.mark.parametrize('p, ks, n, rot', SHAPES)
def test_values(p, ks, n, rot):
    import torch
    from nautilus_amd import PoissonDataLikelihood
    k, resp, e, b, s = problem(p, ks, n, rot)
    cls = (np.arange(p) + rot) % 6
    # what the case holds, checked on the host
    assert np.all(resp >= 0) and np.all(s > 0)
    assert np.any(resp == 0) or p * ks < 8                   # exact zeros
    assert np.any(~resp.any(1)) or p < 8                     # zero rows
    assert np.any(~resp.any(0)) or ks < 4                    # zero columns
    mu = e * (s @ resp.T) + b
    assert np.all(np.isfinite(mu)) and np.all(mu > 0)
    ratio = mu[:, k > 0] / k[k > 0]
    for c, have in ((0, np.any(k == 0)), (2, np.any(k[cls == 2] > 5e6)),
                    (3, ratio.size and np.any(ratio < 1e-10)),
                    (4, ratio.size and np.any(ratio > 1e10))):
        assert bool(have) == bool(np.any(cls == c)), c
    assert np.any(e != 1.0) and np.all(b > 0)
    if p >= 6:
        assert np.all(np.isin(np.arange(6), cls))
        # both log branches
        assert np.any(np.abs(ratio - 1) < 0.5)
        assert np.any(np.abs(ratio - 1) >= 0.5)
    raw = PoissonDataLikelihood(identity, k, exposure=e, background=b,
                                normalised=False, response=resp)
    d = raw.numpy_deviance(s)
    twin = raw.numpy_from_model(s)
    assert np.all(np.isfinite(twin))
    tol = budget(k, resp, e, b, s, d, fold_errors=2)
    st = torch.from_numpy(s).cuda()
    out = raw.from_model(st)
    assert out.is_cuda and out.dtype == torch.float64 and out.shape == (n,)
    got = out.cpu().numpy()
    used = np.abs(got - twin) / np.where(tol > 0, tol, 1.0)
    print('P = %d, K = %d, n = %d, rot = %d: largest used fraction of the '
          'bound %.3g' % (p, ks, n, rot, used.max()))
    assert np.all(np.isfinite(got))
    assert np.all(np.abs(got - twin) <= tol), used.max()
    # the constant joins with one subtraction: log_const - sum, bit for bit
    like = PoissonDataLikelihood(identity, k, exposure=e, background=b,
                                 response=resp)
    assert like.log_const != 0.0 or np.all(k <= 1)
    assert np.array_equal(like.from_model(st).cpu().numpy(),
                          like.log_const - (-got))


@pytest.mark.parametrize('p', [3, 17, 257])
def test_identity_response_against_the_unfolded_kernel(p):
    """With R = I the accumulators are the source values themselves (1 s +
    zeros, exact), so every mu and every term D is the one
    ``nb_poisson_loglike`` forms.  The SUMS are not bit-identical in general:
    that kernel adds a row's terms over column blocks and the lanes 1, 2, 4,
    ... apart, this one over the four registers, the row tiles, the panels,
    the lanes 16 and 32 apart and the wavefronts.  So the two agree within
    twice the summation part of the bound (P eps sum_j D each), and the
    flagged rows agree exactly."""
    import torch
    from nautilus_amd import PoissonDataLikelihood
    k, resp, e, b, s = problem(p, p, 1000, eye=True)
    fold = PoissonDataLikelihood(identity, k, exposure=e, background=b,
                                 response=resp)
    flat = PoissonDataLikelihood(identity, k, exposure=e, background=b)
    st = torch.from_numpy(s).cuda()
    got = fold.from_model(st).cpu().numpy()
    want = flat.from_model(st).cpu().numpy()
    tol = 2 * p * EPS * flat.numpy_deviance(s).sum(1) + \
        2 * EPS * np.abs(want)                     # log_const - sum, rounded
    print('P = %d: %d of 1000 rows bit-identical, largest used fraction %.3g'
          % (p, int(np.sum(got == want)), (np.abs(got - want) / tol).max()))
    assert np.all(np.isfinite(got))
    assert np.all(np.abs(got - want) <= tol)
    dirty = st.clone()
    dirty[5, p - 1] = float('nan')
    dirty[6, 0] = -1.0 - b[0] / e[0]
    a, c = fold.from_model(dirty), flat.from_model(dirty)
    assert bool(torch.isnan(a[5])) and bool(torch.isnan(a[6]))
    assert torch.equal(torch.isnan(a), torch.isnan(c))


@pytest.mark.parametrize('p, ks', [(3, 5), (257, 33), (1025, 130)])
def test_rows_bit_for_bit(p, ks):
    """A row's bits are those it has alone, inside batches of 17, 4097 and
    16 400 (the larger block of points) at different positions, with ld = K
    and ld = K + 5, on any stream, from one handle on two streams."""
    import torch
    from nautilus_amd import PoissonDataLikelihood
    k, resp, e, b, s = problem(p, ks, 4097)
    like = PoissonDataLikelihood(identity, k, exposure=e, background=b,
                                 response=resp)
    big = torch.from_numpy(s).cuda()
    full = like.from_model(big)
    assert bool(torch.isfinite(full).all())
    for off in (0, 1, 777, 4080):
        sub = big[off:off + 17]
        assert sub.data_ptr() == big.data_ptr() + off * ks * 8   # a view
        assert torch.equal(like.from_model(sub), full[off:off + 17]), off
        for r in (off, off + 16):
            assert torch.equal(like.from_model(big[r:r + 1]), full[r:r + 1])
    # the same rows at other positions of a batch
    perm = torch.from_numpy(np.random.default_rng(p).permutation(4097)).cuda()
    assert torch.equal(like.from_model(big[perm]), full[perm])
    assert like.from_model(big[:0]).shape == (0,)
    # a batch that is launched with the larger block of points
    idx = torch.arange(16400, device='cuda') * 5 % 4097
    assert torch.equal(like.from_model(big[idx]), full[idx])
    # a column slice of a wider tensor: rows K + 5 doubles apart
    wide = torch.from_numpy(
        np.random.default_rng(p).normal(size=(4097, ks + 5))).cuda()
    wide[:, 2:2 + ks] = big
    view = wide[:, 2:2 + ks]
    assert view.data_ptr() == wide.data_ptr() + 2 * 8
    assert view.stride() == (ks + 5, 1)
    assert torch.equal(like.from_model(view), full)
    table = like._table()
    assert table.n_data == p and table.n_source == ks
    assert torch.equal(table.loglike(view, ld=ks + 5), full)
    assert torch.equal(table.loglike(big, ld=ks), full)
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
    # one handle on two streams
    torch.cuda.synchronize()
    outs = []
    for st in (torch.cuda.Stream(), torch.cuda.Stream()):
        with torch.cuda.stream(st):
            outs.append(like(big))
    torch.cuda.synchronize()
    assert list(like._tables) == [torch.cuda.current_device()]
    assert torch.equal(outs[0], full) and torch.equal(outs[1], full)


@functools.lru_cache(maxsize=None)
def _edge_problem(p, ks):
    """R >= 0 except one entry; source column K - 1 meets zeros only; bin 1
    sees source column 0 alone, has k > 0 and no background; bin 2 carries
    the negative entry, at source column 2."""
    rng = np.random.default_rng(31 * p + ks)
    resp = 0.1 + rng.random((p, ks))
    resp[:, ks - 1] = 0.0
    resp[1] = 0.0
    resp[1, 0] = 0.75
    resp[2, 2] = -0.01
    e = 0.5 + rng.random(p)
    b = 1.0 + rng.random(p)
    b[1] = 0.0
    s = 0.5 + rng.random((100, ks))
    k = rng.poisson(e * (s[0] @ resp.T) + b).astype(float) + 1.0
    k[0] = 0.0
    return k, resp, e, b, s


@pytest.mark.parametrize('p, ks', [(17, 5), (257, 33), (1025, 130)])
def test_edge_rows(p, ks):
    import torch
    from nautilus_amd import PoissonDataLikelihood
    k, resp, e, b, s = _edge_problem(p, ks)
    assert not resp[:, ks - 1].any() and k[1] > 0 and b[1] == 0
    like = PoissonDataLikelihood(identity, k, exposure=e, background=b,
                                 response=resp)
    clean = torch.from_numpy(s.copy()).cuda()
    want = like.from_model(clean)
    assert bool(torch.isfinite(want).all())
    dirty = clean.clone()
    dirty[3, 0] = 0.0                              # mu = 0 in bin 1, k > 0
    dirty[11, 1] = -1e300                          # negative s: negative mu
    dirty[12, 2] = 1e6                             # negative R: negative mu
    dirty[40, 0] = float('nan')
    dirty[41, ks - 2] = float('inf')
    dirty[42, 1] = float('-inf')
    dirty[43, ks - 1] = float('nan')               # meets zeros of R only
    dirty[44, ks - 1] = float('inf')
    dirty[45, ks - 1] = float('-inf')
    dirty[77, 0] = 0.0                             # -inf and NaN together
    dirty[77, 3] = float('nan')
    dirty[99, 0] = 0.0
    dirty[99, ks - 1] = float('inf')
    mu12 = e * (dirty[12].cpu().numpy() @ resp.T) + b
    assert mu12[2] < 0 and np.all(np.delete(mu12, 2) > 0)
    out = like.from_model(dirty)
    assert float(out[3]) == -np.inf
    nan_rows = (11, 12, 40, 41, 42, 43, 44, 45, 77, 99)
    for i in nan_rows:
        assert bool(torch.isnan(out[i])), i
    keep = torch.ones(100, dtype=torch.bool, device='cuda')
    keep[[3] + list(nan_rows)] = False
    assert torch.equal(out[keep], want[keep])
    twin = like.numpy_from_model(dirty.cpu().numpy())
    assert np.array_equal(np.isnan(twin), torch.isnan(out).cpu().numpy())
    assert np.array_equal(np.isneginf(twin), torch.isinf(out).cpu().numpy())
    # a whole zero row of R with no background and k > 0: every row is -inf,
    # NaN where a source value is not finite
    dead = resp.copy()
    dead[1] = 0.0
    gone = PoissonDataLikelihood(identity, k, exposure=e, background=b,
                                 response=dead)
    rows = clean[:20].clone()
    rows[7, ks - 1] = float('nan')
    out = gone.from_model(rows)
    twin = gone.numpy_from_model(rows.cpu().numpy())
    assert bool(torch.isnan(out[7])) and int(torch.isinf(out).sum()) == 19
    assert bool((out[torch.isinf(out)] < 0).all())
    assert np.array_equal(np.isnan(twin), torch.isnan(out).cpu().numpy())
    assert np.array_equal(np.isneginf(twin), torch.isinf(out).cpu().numpy())
    # the same row with k = 0 contributes nothing: finite
    k0 = k.copy()
    k0[1] = 0.0
    fine = PoissonDataLikelihood(identity, k0, exposure=e, background=b,
                                 response=dead, normalised=False)
    got = fine.from_model(clean[:20]).cpu().numpy()
    d = fine.numpy_deviance(s[:20])
    assert np.all(d[:, 1] == 0.0) and np.all(np.isfinite(got))
    tol = budget(k0, dead, e, b, s[:20], d, fold_errors=2)
    assert np.all(np.abs(got - fine.numpy_from_model(s[:20])) <= tol)


def test_argument_errors_carry_err_arg():
    import ctypes
    import torch
    from nautilus_amd import _lib, device

    def code(*args, **kw):
        with pytest.raises(_lib.NativeError) as err:
            device.FoldedPoissonTable(*args, **kw)
        assert str(err.value)
        return err.value.code

    k = np.array([0.0, 2.0, 5.5])
    r = np.array([[1.0, 0.0], [0.5, -2.0], [0.0, 0.0]])
    one = np.ones(3)
    table = device.FoldedPoissonTable(k, r)
    assert table.n_data == 3 and table.n_source == 2
    assert device.FoldedPoissonTable(k, r, one, 0 * one,
                                     log_const=-3.0).n_data == 3
    # counts, exposure, background, constant: the rules of nb_poisson_create
    assert code(np.zeros(0), np.zeros((0, 2))) == _lib.ERR_ARG
    assert code(k, np.zeros((3, 0))) == _lib.ERR_ARG
    for bad in (np.nan, np.inf, -0.5, 1e-310):
        assert code(np.r_[1.0, bad, 1.0], r) == _lib.ERR_ARG
    for bad in (0.0, -1.0, np.nan, np.inf):
        assert code(k, r, exposure=np.r_[1.0, bad, 1.0]) == _lib.ERR_ARG
    for bad in (-1e-9, np.nan, np.inf):
        assert code(k, r, background=np.r_[0.0, bad, 0.0]) == _lib.ERR_ARG
    assert code(k, r, log_const=np.nan) == _lib.ERR_ARG
    assert code(k, r, log_const=-np.inf) == _lib.ERR_ARG
    # a non-finite response entry
    for bad in (np.nan, np.inf, -np.inf):
        dirty = r.copy()
        dirty[2, 1] = bad
        assert code(k, dirty) == _lib.ERR_ARG
    # NULL counts, NULL response, NULL out, ld_response < n_src
    lib = _lib.load()
    dp = _lib.c_double_p
    h = ctypes.c_void_p()
    kp, rp = k.ctypes.data_as(dp), r.ctypes.data_as(dp)
    assert lib.nb_fold_poisson_create(3, 2, None, rp, 2, None, None, 0.0,
                                      ctypes.byref(h)) == _lib.ERR_ARG
    assert lib.nb_fold_poisson_create(3, 2, kp, None, 2, None, None, 0.0,
                                      ctypes.byref(h)) == _lib.ERR_ARG
    assert lib.nb_fold_poisson_create(3, 2, kp, rp, 2, None, None, 0.0,
                                      None) == _lib.ERR_ARG
    assert lib.nb_fold_poisson_create(3, 2, kp, rp, 1, None, None, 0.0,
                                      ctypes.byref(h)) == _lib.ERR_ARG
    # rows of the response ld_response apart
    padded = np.full((3, 4), np.nan)
    padded[:, :2] = r
    assert lib.nb_fold_poisson_create(
        3, 2, kp, padded.ctypes.data_as(dp), 4, None, None, 0.0,
        ctypes.byref(h)) == 0
    s = torch.tensor([[1.0, 0.25], [3.0, 0.5], [0.5, 0.125], [2.0, 0.0]],
                     dtype=torch.float64, device='cuda')
    out = torch.empty(4, dtype=torch.float64, device='cuda')
    assert lib.nb_fold_poisson_loglike(h, s.data_ptr(), 2, 4, out.data_ptr(),
                                       None) == 0
    torch.cuda.synchronize()
    assert torch.equal(out, table.loglike(s))
    assert lib.nb_fold_poisson_destroy(h) == 0
    # the sizes, checked before any array is read: the pointers of the
    # three-bin problem stand in for arrays that are never touched
    for p, ks in ((0, 2), (3, 0), ((1 << 20) + 1, 1), (1, (1 << 20) + 1),
                  (1 << 20, 17), (4097, 4096), (-1, 2), (3, -1)):
        assert lib.nb_fold_poisson_create(p, ks, kp, rp, max(ks, 1), None,
                                          None, 0.0, ctypes.byref(h)) \
            == _lib.ERR_ARG, (p, ks)
    tall = device.FoldedPoissonTable(np.zeros(1 << 20),
                                     np.zeros((1 << 20, 16)))
    assert tall.n_data == 1 << 20 and tall.n_source == 16
    del tall
    # ld < n_src counts from the second row on
    with pytest.raises(_lib.NativeError) as err:
        table.loglike(s, ld=1)
    assert err.value.code == _lib.ERR_ARG and str(err.value)
    assert table.loglike(s, ld=2).shape == (4,)
    assert torch.equal(table.loglike(s[:1], ld=0), table.loglike(s)[:1])
    # NULL pointers with n > 0, and none needed for n = 0
    assert lib.nb_fold_poisson_loglike(table._h, None, 2, 4, out.data_ptr(),
                                       None) == _lib.ERR_ARG
    assert lib.nb_fold_poisson_loglike(table._h, s.data_ptr(), 2, 4, None,
                                       None) == _lib.ERR_ARG
    assert lib.nb_fold_poisson_loglike(None, s.data_ptr(), 2, 4,
                                       out.data_ptr(), None) == _lib.ERR_ARG
    assert lib.nb_fold_poisson_loglike(table._h, s.data_ptr(), 2, -1,
                                       out.data_ptr(), None) == _lib.ERR_ARG
    assert lib.nb_fold_poisson_loglike(table._h, None, 2, 0, None, None) == 0
    assert lib.nb_fold_poisson_destroy(None) == 0
    # shapes that do not fit together never reach the library
    with pytest.raises(ValueError):
        device.FoldedPoissonTable(k, r[:2])
    with pytest.raises(ValueError):
        device.FoldedPoissonTable(k, r[:, 0])
    with pytest.raises(ValueError):
        device.FoldedPoissonTable(k, r, exposure=np.ones(4))
    with pytest.raises(ValueError):
        device.FoldedPoissonTable(k, r, background=np.zeros(2))
    with pytest.raises(ValueError):
        device.FoldedPoissonTable(k.reshape(3, 1), r)


def test_from_model_layout_rules():
    import torch
    from nautilus_amd import PoissonDataLikelihood
    k, resp, e, b, s = problem(17, 5, 1000)
    like = PoissonDataLikelihood(identity, k, exposure=e, background=b,
                                 response=resp)
    st = torch.from_numpy(s).cuda()
    with pytest.raises(ValueError):
        like.from_model(st[:, :4])
    with pytest.raises(ValueError):
        like.from_model(st[0])
    with pytest.raises(ValueError):
        like.from_model(st.float())
    with pytest.raises(ValueError):
        like.from_model(torch.ones(4, 17, dtype=torch.float64, device='cuda'))
    want = like.from_model(st)
    # anything but unit-stride rows is copied, and gives the same bits
    turned = st.t().contiguous().t()
    assert turned.stride() == (1, 1000)
    assert torch.equal(like.from_model(turned), want)
    twice = torch.stack([st, st], dim=2)[:, :, 0]       # stride(1) == 2
    assert twice.stride(1) == 2
    assert torch.equal(like.from_model(twice), want)
    # numpy in, numpy out
    out = like.from_model(s)
    assert isinstance(out, np.ndarray) and out.dtype == np.float64
    assert np.array_equal(out, want.cpu().numpy())
    called = like(s)                                    # the identity model
    assert isinstance(called, np.ndarray)
    assert np.array_equal(called, out)
    assert like(st).is_cuda and torch.equal(like(st), want)


THETA_MAX = 150.0


@functools.lru_cache(maxsize=None)
def _rates_problem():
    """The three rates of test_sampler_recovers_rates
    (test_poisson_likelihood_gpu.py), each seen by a group of eight bins
    with exposures between 1/2 and 3/2 -- here through a (24, 3) response in
    which bin j of group g sees source g with a weight r_j between 1/2 and
    3/2: counts drawn once from the rates (5, 20, 80)."""
    rng = np.random.default_rng(2026)
    group = np.repeat(np.arange(3), 8)
    e = 0.5 + rng.random(24)
    r = 0.5 + rng.random(24)
    resp = np.zeros((24, 3))
    resp[np.arange(24), group] = r
    k = rng.poisson(np.array([5.0, 20.0, 80.0])[group] * e * r).astype(float)
    return group, e, r, resp, k


def _run_rates():
    from scipy import stats
    from nautilus_amd import PoissonDataLikelihood, Prior, Sampler
    group, e, r, resp, k = _rates_problem()
    prior = Prior()
    for name in 'abc':
        prior.add_parameter(name, dist=stats.uniform(0.0, THETA_MAX))
    assert prior.device                  # transformed on the GPU
    like = PoissonDataLikelihood(identity, k, exposure=e, response=resp)
    s = Sampler(prior, like, pass_dict=False, n_live=1000, n_networks=2,
                vectorized=True, seed=0)
    s.run(n_eff=5000, discard_exploration=True)
    return like, s


def test_sampler_recovers_rates():
    """Evidence and posterior means in the settings, the evidence band and
    the mean tolerance of test_sampler_recovers_rates of
    test_poisson_likelihood_gpu.py: each rate's posterior is
    Gamma(K_g + 1, E_g) cut at theta_max, K_g the group's summed counts and
    E_g = sum_j e_j r_j."""
    from scipy.special import gammainc, gammaln
    group, e, r, resp, k = _rates_problem()
    like, s = _run_rates()
    assert like.n_source == 3 and like.n_data == 24
    analytic, mean, sd = 0.0, np.empty(3), np.empty(3)
    for g in range(3):
        kg, eg = k[group == g], (e * r)[group == g]
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
