"""Every instantiation of the fused Gaussian-mixture likelihood
(``nb_mixture_loglike``, nautilus_amd/csrc/nb_mixture.hip): 8 tile counts x 3
trimming classes x the resident and the streamed form, against the long
double reference of mixture_cases.py under its derived bound; several rounds
of the loop over points; the edges of the running logsumexp; non-finite rows;
the stores of a ragged last group.  (The cases are checked on the CPU in
test_mixture_cases.py.)"""

import ctypes as C

import numpy as np
import pytest

import mixture_cases as mc

pytestmark = pytest.mark.gpu


def _table(means, chol_inv, log_coef):
    from nautilus_amd import device
    return device.MixtureTable(means, chol_inv, log_coef)


def _dev(x):
    """A cuda tensor of a (read-only) array of the case tables."""
    import torch
    return torch.from_numpy(np.array(x, dtype=np.float64, order='C')).cuda()


def _run(table, x):
    import torch
    out, lab = table.loglike(_dev(x), labels=True)
    assert out.is_cuda and out.dtype == torch.float64 and \
        out.shape == (len(x),)
    assert lab.is_cuda and lab.dtype == torch.int32 and lab.shape == (len(x),)
    return out.cpu().numpy(), lab.cpu().numpy()


def _check(out, lab, ref, what, rows_left_out=1e-3):
    """Every value inside the bound of its row, every label the reference's
    wherever the reference decides it."""
    values, bound, terms, term_bound = ref
    assert np.all(np.isfinite(out)), what
    used = np.abs(out - values) / bound
    print('%s: largest used fraction of the bound %.3g' % (what, used.max()))
    assert np.all(used <= 1.0), (what, used.max())
    label, clear = mc.clear_labels(terms, term_bound)
    print('%s: rows left out of the label check: %d' % (what, np.sum(~clear)))
    assert np.mean(~clear) <= rows_left_out
    assert np.array_equal(lab[clear], label[clear]), what


# the largest count whose records fit 160 KB of LDS, DT = 1..8 (nb_layout.h,
# nb_mixture_record: 384, 896, 1664, 2688, 3968, 5504, 7296, 9472 doubles)
LARGEST_RESIDENT = (53, 22, 12, 7, 5, 3, 2, 2)


def _expect_shape(d, k):
    """The instantiation a case is meant for, restated from n_dim and the
    count alone: a launcher that changes its rules fails here instead of
    emptying the sweep."""
    from nautilus_amd import device
    dt = -(-d // 16)
    resident = k <= LARGEST_RESIDENT[dt - 1]
    kl, small = {'full': (4 * dt, False), 'small': (4 * dt - 2, True),
                 'trimmed': (4 * dt - 2, False)}[mc.trim_class(d)]
    tpw = 4 if dt <= 2 else 2 if dt <= 4 else 1
    shape = device.mixture_launch_shape(d, k)
    assert shape[:5] == (dt, kl, small, tpw, resident), shape
    return shape


# ---- A: every instantiation -------------------------------------------------
@pytest.mark.parametrize('d, k', mc.CASES,
                         ids=['%d-%d' % c for c in mc.CASES])
def test_values_every_instantiation(d, k):
    dt, kl, small, _, resident, _ = _expect_shape(d, k)
    means, chol_inv, log_coef, x = mc.case(d, k)
    out, lab = _run(_table(means, chol_inv, log_coef), x)
    _check(out, lab, mc.case_reference(d, k),
           'DT %d, %s, %s, n_dim %d, K %d' % (
               dt, mc.trim_class(d), 'resident' if resident else 'streamed',
               d, k))


# ---- B: several rounds of the loop over points ------------------------------
@pytest.mark.parametrize('d, k', mc.ROUND_CASES,
                         ids=['%d-%d' % c for c in mc.ROUND_CASES])
def test_rounds_bit_for_bit(d, k):
    """A batch of three rounds -- the middle one starts from a record 0 that
    was fetched while the round before it was still multiplying, and fetches
    it again; the last has one full group, one of 5 rows and idle wavefronts
    -- gives the bits of the same rows evaluated in a single round, also when
    it starts one row later."""
    import torch
    from nautilus_amd import device
    tpw, resident = device.mixture_launch_shape(d, k)[3:5]
    assert resident == (k == 3)
    n = mc.round_rows(d, k)
    assert len(mc.rounds_of(d, k, n)) == len(mc.rounds_of(d, k, n - 1)) == 3
    assert len(mc.rounds_of(d, k, mc.ROUND_BASE)) == 1
    means, chol_inv, log_coef, x = mc.case(d, k, False, mc.ROUND_BASE // 2 + 1)
    x = x[:mc.ROUND_BASE]
    table = _table(means, chol_inv, log_coef)
    base = _dev(x)
    small, small_lab = table.loglike(base, labels=True)
    want, _ = mc.twin(means, chol_inv, log_coef, x)
    assert np.allclose(small.cpu().numpy(), want, rtol=mc.RTOL, atol=mc.ATOL)
    reps = -(-n // mc.ROUND_BASE)
    big = base.repeat(reps, 1)[:n]
    assert big.shape == (n, d) and big.is_contiguous()
    want, want_lab = small.repeat(reps)[:n], small_lab.repeat(reps)[:n]
    out, lab = table.loglike(big, labels=True)
    assert torch.equal(out, want)
    assert torch.equal(lab, want_lab)
    shifted = big[1:]
    assert shifted.data_ptr() == big.data_ptr() + d * 8     # a view
    out, lab = table.loglike(shifted, labels=True)
    assert torch.equal(out, want[1:])
    assert torch.equal(lab, want_lab[1:])


# ---- C: the edges of the running logsumexp ----------------------------------
FOLD_DIMS = (6, 38, 70)            # 4, 2 and 1 tiles per wavefront


def _fold_cases():
    return [pytest.param(d, k, id='%d-%d' % (d, k)) for d in FOLD_DIMS
            for k in (mc.k_resident(d), mc.k_streamed(d))]


def _one_component(d):
    """One component of a milder condition number than the sweep's and 300
    points: every |term| stays below 2^22, where doubles are less than 5e-10
    apart -- so raising a coefficient by 1e-9 raises the rounded term."""
    means, covs, w = mc.problem(d, 1, 31 * d, cond=10.0)
    x = mc.points(means, covs, w, 31 * d, 150)
    chol_inv, log_coef = mc.table_arrays(means, covs, w)
    return means, chol_inv, log_coef, x


@pytest.mark.parametrize('d, k', _fold_cases())
def test_fold_edges(d, k):
    """``log_coef`` goes straight to the table, so coefficients that no weight
    could express are allowed.

    1. K copies of one component: the terms of a row are K times the same
       double, the label is the first index (the strict ``>`` of the fold) and
       the value is within the bound of the reference.  With the coefficient
       of one copy raised by 1e-9 every label is that copy's index.
    2. The other copies 2000 lower: exp(-2000) is 0 on either branch of the
       fold, so the result is bit for bit that of the dominant component
       alone.
    3. Overlapping components (several terms of similar size in every row) in
       a random order: the terms keep
       their bits, so both results are the kernel's logsumexp of the same K
       doubles and each is within ``fold_bound`` of the exact one: they differ
       by at most the sum of the two bounds."""
    import torch
    _expect_shape(d, k)
    mu, w_inv, coef, x = _one_component(d)
    means = np.repeat(mu, k, axis=0)
    chol_inv = np.repeat(w_inv, k, axis=0)
    log_coef = np.repeat(coef, k)
    ref = mc.reference(means, chol_inv, log_coef, x)
    assert np.abs(np.asarray(ref[2], float)).max() < 2.0**22
    out, lab = _run(_table(means, chol_inv, log_coef), x)
    assert np.all(lab == 0)
    _check(out, lab, (ref[0], ref[1], ref[2][:1], ref[3][:1]),
           'n_dim %d, %d identical components' % (d, k))
    alone, alone_lab = _table(mu, w_inv, coef).loglike(
        _dev(x), labels=True)
    assert not bool(alone_lab.any())
    for at in (0, k // 2, k - 1):
        raised = log_coef.copy()
        raised[at] += 1e-9
        out, lab = _run(_table(means, chol_inv, raised), x)
        assert np.all(lab == at), (at, np.unique(lab))
        values, bound = mc.reference(means, chol_inv, raised, x)[:2]
        assert np.all(np.abs(out - values) <= bound), at
        # 2: everything else 2000 below copy `at`
        lowered = log_coef - 2000.0
        lowered[at] = log_coef[at]
        got, got_lab = _table(means, chol_inv, lowered).loglike(
            _dev(x), labels=True)
        assert torch.equal(got, alone), at
        assert bool((got_lab == at).all()), at
    # 3
    means, chol_inv, log_coef, x = mc.case(d, k, True)
    _, _, terms, term_bound = mc.case_reference(d, k, True)
    out, lab = _run(_table(means, chol_inv, log_coef), x)
    rng = np.random.default_rng(d + k)
    perm = rng.permutation(k)
    while np.array_equal(perm, np.arange(k)):
        perm = rng.permutation(k)
    out_p, lab_p = _run(_table(means[perm], chol_inv[perm], log_coef[perm]),
                        x)
    label, clear = mc.clear_labels(terms, term_bound)
    assert np.mean(~clear) <= 1e-3
    assert np.array_equal(perm[lab_p][clear], label[clear])
    assert np.array_equal(lab[clear], label[clear])
    limit = mc.fold_bound(k, out) + mc.fold_bound(k, out_p)
    used = np.abs(out - out_p) / limit
    print('n_dim %d, K %d permuted: largest used fraction of the fold bound '
          '%.3g' % (d, k, used.max()))
    assert np.all(used <= 1.0)


@pytest.mark.parametrize('k', [4095, 4096])
def test_fold_edges_at_the_component_limit(k):
    """The largest counts the table takes, odd and even, streamed."""
    assert not _expect_shape(3, k)[4]
    means, chol_inv, log_coef, x = mc.case(3, k, False, 50)
    out, lab = _run(_table(means, chol_inv, log_coef), x)
    assert 0 <= lab.min() and lab.max() < k
    _check(out, lab, mc.case_reference(3, k, False, 50),
           'n_dim 3, K %d' % k, rows_left_out=1.0)


# ---- D: non-finite rows -----------------------------------------------------
# n_dim 1 (a loop of its own in the loads); small, trimmed and full, each with
# an odd and an even n_dim, over 4, 2 and 1 tiles per wavefront
NON_FINITE_DIMS = (1, 3, 20, 37, 70, 111, 128)
BAD_ROWS = (0, 37, 97, 99)         # first; inside a tile; the ragged tail of
#                                    100 rows (96..99) and its last row


@pytest.mark.parametrize('d, k', [
    pytest.param(d, k, id='%d-%d' % (d, k)) for d in NON_FINITE_DIMS
    for k in (mc.k_resident(d), mc.k_streamed(d))])
def test_non_finite_stays_in_its_row(d, k):
    """A NaN or an infinity in a row makes that row's value NaN or -inf,
    never finite and never +inf, and changes no bit of the value or the label
    of any other row.  (The padding slots of a point's operand hold elements
    of its own row, which meet exact zeros of the matrix: 0 x inf = NaN stays
    in the column of the point.)"""
    import torch
    _expect_shape(d, k)
    means, chol_inv, log_coef, x = mc.case(d, k, False, 50)
    assert x.shape == (100, d)
    table = _table(means, chol_inv, log_coef)
    clean = _dev(x)
    want, want_lab = table.loglike(clean, labels=True)
    assert bool(torch.isfinite(want).all())
    keep = torch.ones(100, dtype=torch.bool, device='cuda')
    keep[list(BAD_ROWS)] = False
    seen = set()
    for value in (float('nan'), float('inf'), float('-inf')):
        for f in sorted({0, d // 2, d - 1}):
            dirty = clean.clone()
            dirty[list(BAD_ROWS), f] = value
            out, lab = table.loglike(dirty, labels=True)
            bad = out[~keep]
            assert bool((torch.isnan(bad) | (bad == float('-inf'))).all()), \
                (value, f, bad)
            assert torch.equal(out[keep], want[keep]), (value, f)
            assert torch.equal(lab[keep], want_lab[keep]), (value, f)
            seen |= {'nan' if np.isnan(v) else '-inf'
                     for v in bad.cpu().numpy()}
    print('n_dim %d, K %d: bad rows give %s' % (d, k, sorted(seen)))


# ---- E: the stores of a ragged last group -----------------------------------
SENTINEL = -7.25e300
SENTINEL_LABEL = -77


@pytest.mark.parametrize('d, k', _fold_cases())
def test_nothing_is_written_behind_the_batch(d, k):
    """``out`` and ``label`` of n + 64 elements keep their sentinels behind
    element n - 1; ``label = NULL`` gives the same bits; n = 0 touches
    nothing."""
    import torch
    from nautilus_amd import _lib
    from nautilus_amd.device import _ptr, _stream
    lib = _lib.load()
    means, chol_inv, log_coef, x = mc.case(d, k)
    table = _table(means, chol_inv, log_coef)
    xs = _dev(x)
    full, full_lab = table.loglike(xs, labels=True)
    for n in (0, 1, 15, 16, 17, 63, 65, 600):
        out = torch.full((n + 64,), SENTINEL, dtype=torch.float64,
                         device='cuda')
        lab = torch.full((n + 64,), SENTINEL_LABEL, dtype=torch.int32,
                         device='cuda')
        plain = out.clone()
        _lib.check(lib.nb_mixture_loglike(table._h, _ptr(xs), n, _ptr(out),
                                          _ptr(lab), _stream()))
        _lib.check(lib.nb_mixture_loglike(table._h, _ptr(xs), n, _ptr(plain),
                                          C.c_void_p(None), _stream()))
        torch.cuda.synchronize()
        assert torch.equal(out[:n], full[:n]), n
        assert torch.equal(lab[:n], full_lab[:n]), n
        assert bool((out[n:] == SENTINEL).all()), n
        assert bool((lab[n:] == SENTINEL_LABEL).all()), n
        assert torch.equal(plain, out), n
