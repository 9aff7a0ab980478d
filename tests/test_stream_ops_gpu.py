"""Stream compaction, shell statistics and the live pool at kernel level:
``nb_compact_rows``, ``nb_shell_stats``, ``nb_live_append`` /
``nb_live_select`` / ``nb_live_stats`` called through the C ABI with tensors
the test owns -- sentinels behind every output, guard bytes behind every work
space -- at the sizes where the kernels change their path (stream_cases.py:
wavefront, workgroup, chunk, the 256-chunk rounds of the scan, the grid cap
of the reductions, the eight passes of the radix selection), against the
plain references of stream_cases.py, which test_stream_cases.py checks on the
CPU.

Counts, thresholds, copied rows and source rows are exact.  The two
logsumexp outputs of ``nb_shell_stats`` are held to rtol = atol = 1e-13
against a long double reference (the band of
test_hip_parity.test_shell_stats_match_reference), the logsumexp of
``nb_live_stats`` to 1e-12 (test_live_gpu.py); every test prints its worst
error as a fraction of the band."""

import ctypes as C

import numpy as np
import pytest

import stream_cases as sc

pytestmark = pytest.mark.gpu

GUARD = 64
NAN_BITS = 0x7ff8dead0000beef          # the sentinel of untouched doubles
inf = np.inf


@pytest.fixture(autouse=True)
def gpu_only():
    import torch
    if not torch.cuda.is_available():
        pytest.skip('no GPU')


def _lib():
    from nautilus_amd import _lib as binding
    return binding, binding.load()


def _ptr(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _stream():
    from nautilus_amd import device
    return device._stream()


def _dev(a):
    import torch
    return torch.from_numpy(np.array(a)).cuda()     # (a copy: a may be frozen)


def _full(n, value, dtype):
    import torch
    return torch.full((n,), value, dtype=dtype, device='cuda')


def _sentinel_doubles(n):
    import torch
    return _full(n, NAN_BITS, torch.int64).view(torch.float64)


def _untouched(t, start):
    """The doubles of ``t`` from ``start`` on still hold the sentinel."""
    import torch
    return bool((t.view(-1).view(torch.int64)[start:] == NAN_BITS).all())


# ---------------------------------------------------------------------------
# nb_compact_rows
# ---------------------------------------------------------------------------
def _compact(x, flags_dev, mask, flip, n, count_only=False):
    """One call with exactly-sized work space.  Returns (counts, out, src,
    intact): ``out`` with n + 2 rows and ``src`` with n + GUARD entries
    holding sentinels, ``intact`` = the guard bytes behind the scratch and the
    words behind the counts are unchanged."""
    import torch
    binding, lib = _lib()
    d = x.shape[1]
    n_scratch = lib.nb_compact_scratch_bytes(n)
    assert n_scratch == ((n + sc.CHUNK - 1) // sc.CHUNK * 2 + 2) * 8
    scratch = _full(n_scratch + GUARD, 0xa5, torch.uint8)
    counts = _full(2 + 2, -7, torch.int64)
    out = src = None
    if not count_only:
        out = _sentinel_doubles((n + 2) * d).view(n + 2, d)
        src = _full(n + GUARD, -1, torch.int64)
    binding.check(lib.nb_compact_rows(
        _ptr(x), _ptr(flags_dev), mask, flip, n, d, _ptr(out), _ptr(src),
        _ptr(counts), _ptr(scratch), _stream()))
    intact = bool((scratch[n_scratch:] == 0xa5).all()) and \
        counts[2:].tolist() == [-7, -7]
    return counts[:2].tolist(), out, src, intact


def _check_compaction(n, d, large):
    import torch
    x_host = sc.compact_points(n, d)
    x = _dev(x_host)
    x_bits = x.view(torch.int64)
    unequal = 0
    for mask, flip in sc.MASK_FLIP:
        for name, flags in sc.flag_patterns(n, mask, flip, large):
            case = (n, d, mask, flip, name)
            _, want_src, want_counts = sc.compact_reference(
                x_host[:, :0], flags, mask, flip)
            # the flags are the first n bytes of a longer tensor whose other
            # bytes would be kept, and counted, under this mask and flip
            longer = np.full(n + 4 * GUARD, sc.beyond_byte(flip), np.uint8)
            longer[:n] = flags
            flags_dev = _dev(longer)
            counts, out, src, intact = _compact(x, flags_dev, mask, flip, n)
            assert counts == want_counts.tolist(), case
            assert intact, case
            k = counts[1]
            idx = _dev(want_src)
            assert torch.equal(src[:k], idx), case
            assert bool((src[k:] == -1).all()), case
            # (bit-equal: the rows hold NaN, -0.0 and a denormal)
            assert torch.equal(out.view(torch.int64)[:k], x_bits[idx]), case
            assert _untouched(out, k * d), case
            unequal += counts[0] != counts[1]
            # count-only mode
            counts, _, _, intact = _compact(x, flags_dev, mask, flip, n,
                                            count_only=True)
            assert counts == want_counts.tolist() and intact, case
    assert n == 1 or unequal > 0


@pytest.mark.parametrize('d', sc.COMPACT_SMALL_DIMS)
@pytest.mark.parametrize('n', sc.COMPACT_SMALL_N)
def test_compaction_small(n, d):
    """Every (mask, flip) pair and flag pattern at the edges of a wavefront,
    a round of 256 flags and a chunk, at both ends of the scatter kernel's
    row / column stepping (n_dim 1 ... 128)."""
    _check_compaction(n, d, large=False)


@pytest.mark.parametrize('d', sc.COMPACT_LARGE_DIMS)
@pytest.mark.parametrize('n', sc.COMPACT_LARGE_N)
def test_compaction_across_scan_rounds(n, d):
    """256, 257 and 514 chunks: the scan kernel carries its totals from one
    round of 256 chunks to the next."""
    _check_compaction(n, d, large=True)


def test_compaction_reference_rows_on_the_host():
    """The copied rows once more against ``compact_reference`` itself, on the
    host (the other tests gather the reference rows on the device)."""
    n, d = 2049, 7
    x_host = sc.compact_points(n, d)
    for mask, flip in sc.MASK_FLIP:
        for name, flags in sc.flag_patterns(n, mask, flip):
            rows, _, counts = sc.compact_reference(x_host, flags, mask, flip)
            _, out, _, _ = _compact(_dev(x_host), _dev(flags), mask, flip, n)
            got = out.cpu().numpy()[:counts[1]]
            assert np.array_equal(got.view(np.int64), rows.view(np.int64))


@pytest.mark.parametrize('n', sc.COMPACT_SMALL_N + sc.COMPACT_LARGE_N)
def test_source_rows_are_the_trials_until_the_kth_success(n):
    """The sampler's call (mask = flip = 2, device.compact_rows): the source
    row of the k-th survivor, plus one, is the number of rows examined until
    k rows had their flag clear -- for the first, the middle and the last
    survivor of every pattern, the random ones among them."""
    from nautilus_amd import device
    mask = flip = 2
    x = _dev(np.zeros((n, 3)))
    for name, flags in sc.flag_patterns(n, mask, flip, large=n > 4096):
        clear = (flags & 2) == 0                     # rows the sampler keeps
        trials = np.flatnonzero(clear) + 1           # examined at success k
        out, counts, src = device.compact_rows(x, _dev(flags), mask=mask,
                                               want_index=True, flip=flip)
        c = counts.tolist()
        assert c[1] == len(trials), (n, name)
        assert c[0] == int(np.sum((flags ^ flip) & 1)), (n, name)
        for k in {min(1, c[1]), c[1] // 2, c[1]} - {0}:
            assert int(src[k - 1]) + 1 == trials[k - 1], (n, name, k)
            assert clear[:trials[k - 1]].sum() == k


# ---------------------------------------------------------------------------
# nb_shell_stats
# ---------------------------------------------------------------------------
def _shell_stats(l, threshold):
    """One call with exactly-sized work space; a large value sits behind the
    n inputs.  Returns (out, intact)."""
    import torch
    binding, lib = _lib()
    n = len(l)
    n_scratch = lib.nb_shell_stats_scratch_bytes(n)
    assert n_scratch == min(1024, max(1, (n + 255) // 256)) * 32
    scratch = _full(n_scratch + GUARD, 0xa5, torch.uint8)
    out = _sentinel_doubles(4 + 4)
    l_dev = _dev(np.concatenate([l, np.full(GUARD, 1e300)]))
    binding.check(lib.nb_shell_stats(_ptr(l_dev), n, float(threshold),
                                     _ptr(out), _ptr(scratch), _stream()))
    intact = bool((scratch[n_scratch:] == 0xa5).all()) and _untouched(out, 4)
    return out[:4].cpu().numpy(), intact


def _band_fraction(got, want):
    """|got - want| over the band atol + rtol |want| of np.isclose."""
    if got == want:
        return 0.0
    return abs(got - want) / (sc.LSE_ATOL + sc.LSE_RTOL * abs(want))


@pytest.mark.parametrize('n', sc.LSE_N)
def test_shell_stats_contents_and_thresholds(n):
    worst = [0.0, 0.0]
    for name, l, tie in sc.lse_contents(n):
        sums = sc.lse_reference(l, tie)[:3]       # (once per content)
        for tname, thr in sc.lse_thresholds(l, tie):
            want = sums + (int(np.count_nonzero(l >= thr)),)
            got, intact = _shell_stats(l, thr)
            case = (n, name, tname)
            assert intact, case
            frac = [_band_fraction(got[i], want[i]) for i in (0, 1)]
            print('shell_stats n=%d %s %s: error / band = %.3g, %.3g' % (
                n, name, tname, frac[0], frac[1]))
            worst = [max(w, f) for w, f in zip(worst, frac)]
            assert np.isclose(got[0], want[0], rtol=sc.LSE_RTOL,
                              atol=sc.LSE_ATOL), case
            assert np.isclose(got[1], want[1], rtol=sc.LSE_RTOL,
                              atol=sc.LSE_ATOL), case
            assert got[2] == want[2], case
            assert got[3] == want[3], case
            if tname == 'minus_inf':
                assert got[3] == n, case
            if tname == 'plus_inf':
                assert got[3] == 0, case
    print('shell_stats n=%d worst error / band: logsumexp(l) %.3g, '
          'logsumexp(2l) %.3g' % (n, worst[0], worst[1]))


def test_shell_stats_all_minus_inf_and_through_the_wrapper():
    from nautilus_amd import device
    for n in sc.LSE_N:
        l = np.full(n, -inf)
        got, intact = _shell_stats(l, -inf)
        assert intact and got.tolist() == [-inf, -inf, -inf, n]
        assert _shell_stats(l, 0.0)[0].tolist() == [-inf, -inf, -inf, 0]
        name, l, tie = sc.lse_contents(n)[-1]
        want = sc.lse_reference(l, tie)
        got = device.shell_stats(_dev(l), tie).cpu().numpy()
        assert np.isclose(got[0], want[0], rtol=sc.LSE_RTOL, atol=sc.LSE_ATOL)
        assert np.isclose(got[1], want[1], rtol=sc.LSE_RTOL, atol=sc.LSE_ATOL)
        assert got[2] == want[2] and got[3] == want[3]


@pytest.mark.parametrize('n', sc.LSE_N)
def test_shell_stats_one_nan(n):
    """One NaN anywhere: both sums are NaN, as scipy's logsumexp is (the
    maximum too, as numpy's); the count takes the NaN for below the
    threshold."""
    base = sc.lse_contents(n)[-1][1]
    for at in sc.nonfinite_positions(n):
        l = base.copy()
        l[at] = np.nan
        want = sc.lse_reference(l, -5.0)
        assert np.isnan(want[0]) and np.isnan(want[1])
        got, intact = _shell_stats(l, -5.0)
        assert intact
        assert np.isnan(got[0]) and np.isnan(got[1]) and np.isnan(got[2]), (
            n, at, got)
        assert got[3] == want[3], (n, at)


@pytest.mark.parametrize('n', sc.LSE_N)
def test_shell_stats_one_plus_inf(n):
    """One +inf anywhere: both sums and the maximum are +inf, as scipy's
    logsumexp is."""
    base = sc.lse_contents(n)[-1][1]
    for at in sc.nonfinite_positions(n):
        l = base.copy()
        l[at] = inf
        want = sc.lse_reference(l, inf)
        assert want == (inf, inf, inf, 1)
        got, intact = _shell_stats(l, inf)
        assert intact
        assert got.tolist() == [inf, inf, inf, 1], (n, at, got)


# ---------------------------------------------------------------------------
# nb_live_append
# ---------------------------------------------------------------------------
def _append(l, thr, cap, before):
    """Append the batch ``l`` to a pool of capacity ``cap`` that holds
    ``before`` already.  Returns (pool[:cap], pool_n, overflow, intact)."""
    import torch
    binding, lib = _lib()
    pool = _sentinel_doubles(cap + GUARD)
    pool[:len(before)] = _dev(before)
    words = _full(2 + 2, -7, torch.int32)         # pool_n, overflow, guards
    words[0], words[1] = len(before), 0
    l_dev, thr_dev = _dev(l), _dev(np.array([thr]))
    binding.check(lib.nb_live_append(
        _ptr(l_dev), len(l), _ptr(thr_dev), _ptr(pool), _ptr(words[0:]), cap,
        _ptr(words[1:]), _stream()))
    w = words.tolist()
    intact = _untouched(pool, cap) and w[2:] == [-7, -7]
    return pool[:cap].cpu().numpy(), w[0], w[1], intact


@pytest.mark.parametrize('nan', (False, True), ids=('finite', 'nan'))
@pytest.mark.parametrize('n', sc.APPEND_N)
def test_live_append(n, nan):
    before = np.array([9.5, -2.0, sc.LIVE_TIE, 9.5, 100.0])
    l = sc.live_batch(n, nan)
    tie = sc.LIVE_TIE if n > 4 else l[np.isfinite(l)].max(initial=-inf)
    for thr in (-inf, tie, inf):
        # NaN >= thr is false: never appended; -inf >= -inf: appended
        accepted = l[l >= thr]
        assert thr != -inf or len(accepted) == n - np.isnan(l).sum()
        total = len(before) + len(accepted)
        # room to spare, exactly enough, one place short, half the places
        for cap in sorted({total + 100, total, max(total - 1, len(before)),
                           len(before) + len(accepted) // 2}):
            pool, pool_n, overflow, intact = _append(l, thr, cap, before)
            case = (n, nan, thr, cap)
            assert intact, case
            assert pool_n == total, case             # even beyond cap
            assert overflow == (1 if total > cap else 0), case
            assert np.array_equal(pool[:len(before)], before), case
            got = pool[len(before):min(total, cap)]
            if total <= cap:
                assert np.array_equal(np.sort(got), np.sort(accepted)), case
                assert np.isnan(pool[total:]).all(), case
            else:
                # a full pool holds some of the accepted values, each at
                # most as often as the batch has it
                u, c = np.unique(got, return_counts=True)
                ua, ca = np.unique(accepted, return_counts=True)
                assert np.isin(u, ua).all(), case
                assert np.all(c <= ca[np.searchsorted(ua, u)]), case


# ---------------------------------------------------------------------------
# nb_live_select
# ---------------------------------------------------------------------------
def _select(values, k, cap=None, pool_n=None):
    """Select among ``values[:cap]``.  Returns (stats, thr, kept sorted,
    intact)."""
    import torch
    binding, lib = _lib()
    cap = len(values) if cap is None else cap
    pool_n = len(values) if pool_n is None else pool_n
    pool = _dev(values)
    out = _sentinel_doubles(cap + GUARD)
    words = _full(2 + 2, -7, torch.int32)         # pool_n, out_n, guards
    words[0] = pool_n
    thr = _dev(np.array([123.0, 456.0]))
    stats = _sentinel_doubles(3 + 3)
    binding.check(lib.nb_live_select(
        _ptr(pool), _ptr(words[0:]), cap, k, _ptr(out), _ptr(words[1:]),
        _ptr(thr), _ptr(stats), _stream()))
    w = words.tolist()
    thr = thr.tolist()
    out_n = w[1]
    assert 0 <= out_n <= cap
    intact = _untouched(out, out_n) and _untouched(stats, 3) and \
        w[0] == pool_n and w[2:] == [-7, -7] and thr[1] == 456.0 and \
        torch.equal(pool, _dev(values))
    return (stats[:3].tolist(), thr[0], np.sort(out[:out_n].cpu().numpy()),
            intact)


def _check_select(values, k, case, **kw):
    want_thr, n_gt, n_eq, kept = sc.select_reference(
        values[:kw.get('cap', len(values))], k)
    stats, thr, got, intact = _select(values, k, **kw)
    assert intact, case
    assert stats == [want_thr, n_gt, n_eq], case
    assert thr == want_thr, case
    assert len(got) == n_gt + n_eq, case
    # (bit-equal up to the order, -0.0 and 0.0 apart)
    assert np.array_equal(np.sort(sc.lv_key(got)), np.sort(sc.lv_key(kept))), \
        case


_RADIX = sc.radix_cases()


@pytest.mark.parametrize('name,values,k,j', _RADIX,
                         ids=[c[0] for c in _RADIX])
def test_live_select_decided_in_every_pass(name, values, k, j):
    """Pools whose k-th largest key is decided in pass j of the radix
    selection and no earlier (test_stream_cases.py shows that on the CPU),
    negative and positive; directly and through ``device.LivePool``."""
    from nautilus_amd import device
    _check_select(values, k, name)
    want_thr, n_gt, n_eq, _ = sc.select_reference(values, k)
    assert (n_gt, n_eq) == (k - 1, 1)
    assert device.LivePool(k, [_dev(values)]).select() == (want_thr, n_gt,
                                                           n_eq)


_FURTHER = sc.further_pools()


@pytest.mark.parametrize('name,values,k', _FURTHER,
                         ids=[c[0] for c in _FURTHER])
def test_live_select_signs_zeros_denormals_ties(name, values, k):
    from nautilus_amd import device
    _check_select(values, k, name)
    assert device.LivePool(k, [_dev(values)]).select() == \
        sc.select_reference(values, k)[:3]


@pytest.mark.parametrize('p', sc.SELECT_P)
def test_live_select_random_pools(p):
    values = sc.random_pool(p)
    for k in sc.select_ks(p):
        _check_select(values, k, (p, k))
        if k == p + 1:                    # fewer values than places
            stats, thr, got, _ = _select(values, k)
            assert thr == -inf and stats == [-inf, p, 0] and len(got) == p
    # a pool with -inf entries and fewer finite values than places: the
    # threshold is -inf by selection, the -inf entries are the ties
    mixed = np.concatenate([values, np.full(7, -inf)])
    stats, thr, got, _ = _select(mixed, p + 3)
    assert stats == [-inf, p, 7] and len(got) == p + 7


@pytest.mark.parametrize('p', (256, 1025))
def test_live_select_clips_pool_n_to_the_capacity(p):
    """pool_n counts every accepted value, also those that found no place:
    only the first ``cap`` entries take part."""
    values = np.concatenate([sc.random_pool(p), np.full(50, 1e9)])
    for k in (1, 2, p - 1, p):
        _check_select(values, k, (p, k), cap=p, pool_n=p + 50)
    stats, thr, got, intact = _select(values, p + 1, cap=p, pool_n=p + 50)
    assert intact and thr == -inf and stats == [-inf, p, 0] and len(got) == p


# ---------------------------------------------------------------------------
# nb_live_stats
# ---------------------------------------------------------------------------
def _live_stats(l, thr):
    binding, lib = _lib()
    out = _sentinel_doubles(3 + 3)
    l_dev = _dev(np.concatenate([l, np.full(GUARD, 1e300)]))
    thr_dev = _dev(np.array([thr]))
    binding.check(lib.nb_live_stats(_ptr(l_dev), len(l), _ptr(thr_dev),
                                    _ptr(out), _stream()))
    return out[:3].tolist(), _untouched(out, 3)


@pytest.mark.parametrize('n', sc.STATS_N)
def test_live_stats(n):
    l = sc.live_batch(n)
    top = l.max(initial=-inf)
    worst = 0.0
    for tname, thr in (('minus_inf', -inf), ('tie', sc.LIVE_TIE),
                       ('at_max', top), ('above_max', max(top, 0.0) + 1.0)):
        want = sc.live_stats_reference(l, thr)
        got, intact = _live_stats(l, thr)
        case = (n, tname)
        assert intact, case
        assert got[0] == want[0] and got[2] == want[2], case
        if want[0] == 0:
            assert got[1] == -inf, case
        else:
            err = abs(got[1] - want[1])
            worst = max(worst, err / sc.LIVE_ATOL)
            assert err < sc.LIVE_ATOL, case
        if tname == 'above_max':
            assert got == [0, -inf, 0], case
        if tname == 'minus_inf':
            assert got[2] == np.sum(l == -inf), case
    print('live_stats n=%d worst error / 1e-12: %.3g' % (n, worst))


def test_live_stats_null_batch_and_plus_inf():
    """n = 0 with no batch at all; a +inf above the threshold gives +inf, as
    scipy's logsumexp does; a NaN is neither above nor at the threshold."""
    binding, lib = _lib()
    out, thr_dev = _sentinel_doubles(3), _dev(np.array([0.0]))
    binding.check(lib.nb_live_stats(None, 0, _ptr(thr_dev), _ptr(out),
                                    _stream()))
    assert out.tolist() == [0, -inf, 0]
    for n in (1, 1023, 1025, 70001):
        base = sc.live_batch(n)
        for at in sc.nonfinite_positions(n):
            l = base.copy()
            l[at] = inf
            n_gt = int(np.sum(l > 0.5))
            assert _live_stats(l, 0.5)[0] == [n_gt, inf, np.sum(l == 0.5)]
            assert _live_stats(l, inf)[0] == [0, -inf, 1]
            l[at] = np.nan
            want = sc.live_stats_reference(l, 0.5)
            got = _live_stats(l, 0.5)[0]
            assert got[0] == want[0] and got[2] == want[2]
            assert want[0] == 0 or abs(got[1] - want[1]) < sc.LIVE_ATOL
