"""The references and pools of stream_cases.py, on the CPU: the compaction
reference against a Python loop, the long double logsumexp against scipy and
against rational arithmetic, the restated radix key against the order of the
doubles, and every radix pool against its claim -- the k-th largest key is
decided in the pass it names and in no earlier one, so the device test
(test_stream_ops_gpu.py) reaches all eight passes of ``nb_live_select``."""

from fractions import Fraction

import numpy as np
import pytest
from scipy.special import logsumexp

import stream_cases as sc


# ---- compaction -------------------------------------------------------------
def _compact_loop(x, flags, mask, flip):
    rows, src, c0 = [], [], 0
    for i, f in enumerate(flags.tolist()):
        f ^= flip
        c0 += f & 1
        if f & mask:
            rows.append(x[i])
            src.append(i)
    return rows, src, [c0, len(src)]


@pytest.mark.parametrize('mask,flip', sc.MASK_FLIP)
@pytest.mark.parametrize('n', (1, 257, 2049))
def test_compact_reference_against_a_loop(n, mask, flip):
    x = np.arange(3.0 * n).reshape(n, 3)
    unequal = 0
    for name, flags in sc.flag_patterns(n, mask, flip):
        assert flags.dtype == np.uint8 and flags.shape == (n,)
        rows, src, counts = sc.compact_reference(x, flags, mask, flip)
        want_rows, want_src, want_counts = _compact_loop(x, flags, mask, flip)
        assert src.tolist() == want_src, name
        assert counts.tolist() == want_counts, name
        assert np.array_equal(rows, np.array(want_rows).reshape(-1, 3)), name
        unequal += counts[0] != counts[1]
    # the bits outside the mask are noise: bit 0 differs from the decision
    assert unequal > 0 or n == 1 or (mask, flip) in ((1, 0), (1, 1))


@pytest.mark.parametrize('mask,flip', sc.MASK_FLIP)
@pytest.mark.parametrize('n', sc.COMPACT_SMALL_N + (sc.SCAN_ROWS + 1,))
def test_flag_patterns_keep_what_their_names_say(n, mask, flip):
    pats = dict(sc.flag_patterns(n, mask, flip, large=n > 4096))
    noise = sc.noise_bytes(n)
    for name, keep in sc.keep_patterns(n, large=n > 4096):
        _, src, _ = sc.compact_reference(np.zeros((n, 1)), pats[name], mask,
                                         flip)
        assert np.array_equal(src, np.flatnonzero(keep)), name
        # outside the mask the flags are the noise bytes
        assert np.array_equal((pats[name] ^ flip) & ~np.uint8(mask),
                              noise & ~np.uint8(mask)), name
    for r in (0, n - 1, 63, 64, 255, 256, 2047, 2048, n - 2048):
        assert ('only_row_%d' % r in pats) == (0 <= r < n)
    assert np.array_equal(pats['bytes'], noise)
    if n >= 2047:
        assert len(np.unique(noise)) == 256
    # the byte behind the flags would be kept, and counted for counts[0]
    b = sc.beyond_byte(flip) ^ flip
    assert b & mask and b & 1


# ---- logsumexp --------------------------------------------------------------
_ONE = 1 << 256


def _fix(q):
    """Round a rational to a multiple of 2^-256."""
    return Fraction(round(q * _ONE), _ONE)


def _exp_q(x):
    """exp of a rational x <= 0 to ~2^-240: x / 2^s in (-1, 0], 60 terms of
    the series, s squarings."""
    s = 0
    while abs(x) >= 1:
        x /= 2
        s += 1
    term, total = Fraction(1), Fraction(1)
    for i in range(1, 60):
        term = _fix(term * x / i)
        total += term
    for _ in range(s):
        total = _fix(total * total)
    return total


def _atanh2_q(z):
    """2 atanh(z) = log((1 + z) / (1 - z)) for a rational |z| <= 1/3."""
    term, total, z2 = z, z, z * z
    for i in range(1, 160):
        term = _fix(term * z2)
        total += term / (2 * i + 1)
    return 2 * total


def _log_q(q):
    """log of a rational q >= 1: q = 2^e f with f in [1, 2)."""
    e = 0
    while q >= 2:
        q /= 2
        e += 1
    return e * _atanh2_q(Fraction(1, 3)) + _atanh2_q((q - 1) / (q + 1))


def _logsumexp_q(values):
    m = max(values)
    q = [Fraction(v) - Fraction(m) for v in values if v != -np.inf]
    return Fraction(m) + _log_q(sum(_exp_q(x) for x in q))


_SMALL = [[0.0], [-1.5, -1.5], [0.1, 0.2, 0.3], [-7.0, 0.5, -np.inf, 0.5],
          [1e-3, -1e-3, 0.0, 5.25, -2.75], [-40.0, -3.0, -3.0000000001],
          [700.0, 699.5, 692.0], list(np.linspace(-9.0, 1.0, 23))]


@pytest.mark.parametrize('values', _SMALL, ids=range(len(_SMALL)))
def test_lse_reference_against_rational_arithmetic(values):
    l = np.array(values)
    got = sc.lse_reference(l, 0.0)
    for g, v in ((got[0], l), (got[1], 2 * l)):
        exact = _logsumexp_q(v.tolist())
        assert abs(Fraction(g) - exact) <= Fraction(float(np.spacing(abs(g))))
    assert got[2] == max(values)
    assert got[3] == sum(v >= 0.0 for v in values)
    gt, lse_gt, eq = sc.live_stats_reference(l, 0.5)
    above = [v for v in values if v > 0.5]
    assert gt == len(above) and eq == sum(v == 0.5 for v in values)
    if above:
        assert abs(Fraction(lse_gt) - _logsumexp_q(above)) <= Fraction(
            float(np.spacing(abs(lse_gt))))
    else:
        assert lse_gt == -np.inf


@pytest.mark.parametrize('n', (1, 65, 257, 262145))
def test_lse_reference_against_scipy(n):
    """On the contents of the device test: the long double reference, scipy
    and an exactly rounded sum of double terms agree far inside the 1e-13 the
    device is held to."""
    for name, l, tie in sc.lse_contents(n):
        got = sc.lse_reference(l, tie)
        for g, v in ((got[0], l), (got[1], 2 * l)):
            assert np.isclose(g, logsumexp(v), rtol=2e-15, atol=2e-15), name
            assert np.isclose(g, sc.fsum_logsumexp(v), rtol=2e-15,
                              atol=2e-15), name
        assert got[2] == np.max(l)
        assert 1 <= got[3] == np.sum(l >= tie)
        for tname, thr in sc.lse_thresholds(l, tie):
            assert tname != 'between' or not np.any(l == thr)


def test_lse_reference_edges():
    inf = np.inf
    assert sc.lse_reference(np.array([]), 0.0) == (-inf, -inf, -inf, 0)
    assert sc.lse_reference(np.full(5, -inf), -inf) == (-inf, -inf, -inf, 5)
    assert sc.lse_reference(np.full(5, -inf), 0.0)[3] == 0
    got = sc.lse_reference(np.array([0.0, np.nan, 1.0]), 0.0)
    assert np.isnan(got[0]) and np.isnan(got[1]) and got[3] == 2
    with np.errstate(invalid='ignore'):
        want = logsumexp(np.array([0.0, inf, 1.0]))
    got = sc.lse_reference(np.array([0.0, inf, 1.0]), inf)
    assert got == (inf, inf, inf, 1) and want == inf
    assert sc.live_stats_reference(np.array([]), -inf) == (0, -inf, 0)
    assert sc.live_stats_reference(np.array([-inf, 1.0, 2.0]), 2.0) == (
        0, -inf, 1)
    assert sc.live_stats_reference(np.array([-inf, 1.0]), -inf) == (1, 1.0, 1)


def test_lse_contents_have_their_ties_and_edges():
    for n in sc.LSE_N:
        contents = {name: (l, tie) for name, l, tie in sc.lse_contents(n)}
        assert len(contents) == 10
        for name, (l, tie) in contents.items():
            assert l.shape == (n,) and not np.isnan(l).any(), name
            several = n >= 64 and name not in ('ascending', 'descending') \
                and not name.startswith('finite_')
            assert np.sum(l == tie) >= (2 if several else 1), (n, name)
        assert np.all(np.diff(contents['ascending'][0]) > 0)
        assert np.all(np.diff(contents['descending'][0]) < 0)
        l = contents['max_last'][0]
        assert n == 1 or l[-1] > l[:-1].max()
        l = contents['finite_tail_block'][0]
        at = np.flatnonzero(np.isfinite(l))
        assert len(at) == 1 and at[0] % 256 == 0 and n - at[0] <= 256
        l = contents['wide_range'][0]
        if n >= 255:                      # most terms underflow a double sum
            assert np.mean(np.exp(l - l.max()) < 2.0**-53) > 0.9
        l = contents['half_minus_inf'][0]
        assert n < 4 or 0.2 < np.mean(l == -np.inf) <= 0.5


# ---- the key of the radix selection -----------------------------------------
def _sorted_doubles():
    tiny = 5e-324
    rng = np.random.default_rng(3)
    v = np.concatenate([
        [-np.inf, np.inf, -0.0, 0.0, tiny, -tiny, 2 * tiny, -2 * tiny,
         2.2250738585072014e-308, -2.2250738585072014e-308,
         2.225073858507201e-308, -2.225073858507201e-308,
         1.7976931348623157e308, -1.7976931348623157e308, 1.0, -1.0,
         np.nextafter(1.0, 2), np.nextafter(-1.0, -2)],
        rng.standard_normal(500), -np.exp(rng.uniform(-740, 700, 500)),
        np.exp(rng.uniform(-740, 700, 500)),
        rng.integers(1, 1 << 52, 200).astype(np.uint64).view(np.float64),
        -rng.integers(1, 1 << 52, 200).astype(np.uint64).view(np.float64)])
    return np.sort(np.unique(v))


def test_key_is_strictly_monotone_and_round_trips():
    v = _sorted_doubles()
    # np.unique holds -0.0 and 0.0 for one value: order the two by hand
    zero = np.flatnonzero(v == 0.0)
    assert len(zero) == 1
    v = np.concatenate([v[:zero[0]], [-0.0, 0.0], v[zero[0] + 1:]])
    assert np.signbit(v[zero[0]]) and not np.signbit(v[zero[0] + 1])
    keys = sc.lv_key(v)
    assert keys.dtype == np.uint64
    assert np.all(keys[1:] > keys[:-1])
    back = sc.lv_key_inverse(keys)
    assert np.array_equal(back.view(np.uint64), v.view(np.uint64))
    assert sc.lv_key(np.array([0.0]))[0] == 1 << 63
    assert sc.lv_key(np.array([-0.0]))[0] == (1 << 63) - 1
    assert sc.lv_key(np.array([-np.inf]))[0] == 0x000fffffffffffff
    assert sc.lv_key(np.array([np.inf]))[0] == 0xfff0000000000000
    # without the sign branch the negative values would come out in
    # descending order
    plain = v.view(np.uint64) | np.uint64(1 << 63)
    assert np.all(plain[1:zero[0]] < plain[:zero[0] - 1])


_RADIX = sc.radix_cases()


def test_radix_cases_cover_every_pass_and_both_signs():
    assert sorted({j for _, _, _, j in _RADIX}) == list(range(8))
    for j in range(1, 8):
        signs = {bool(np.all(v < 0)) for _, v, _, jj in _RADIX if jj == j}
        assert signs == {True, False}
    mixed = [v for _, v, _, j in _RADIX if j == 0]
    assert all(np.any(v < 0) and np.any(v > 0) for v in mixed)


@pytest.mark.parametrize('name,values,k,j', _RADIX,
                         ids=[c[0] for c in _RADIX])
def test_radix_pool_is_decided_in_its_pass(name, values, k, j):
    assert not np.isnan(values).any() and not np.isinf(values).any()
    keys = sc.lv_key(values)
    assert len(np.unique(keys)) == len(keys) == sc.RADIX_P
    if j > 0:                        # the top j bytes are shared ...
        assert len(np.unique(keys >> np.uint64(64 - 8 * j))) == 1
    digit = (keys >> np.uint64(56 - 8 * j)) & np.uint64(255)
    assert len(np.unique(digit)) == sc.RADIX_P   # ... byte j differs
    left = sc.candidates_per_pass(values, k)
    assert all(c == sc.RADIX_P for c in left[:j])      # open before pass j
    assert left[j:] == [1] * (8 - j)                   # resolved at pass j
    assert sc.decisive_pass(values, k) == j
    # the key restatement agrees with the order of the doubles
    answer = sc.lv_key_inverse(np.sort(keys)[-k:][:1])[0]
    assert answer == sc.kth_largest(values, k)
    # k = p ends in bin 0 of the decisive pass, k = 1 in bin 255 (1 / 254
    # in pass 0, where 0 and 255 would be NaNs)
    mine = int(digit[values == answer][0])
    if k == sc.RADIX_P:
        assert mine == (1 if j == 0 else 0)
    if k == 1:
        assert mine == (254 if j == 0 else 255)


_FURTHER = sc.further_pools()


@pytest.mark.parametrize('name,values,k', _FURTHER,
                         ids=[c[0] for c in _FURTHER])
def test_further_pools(name, values, k):
    assert not np.isnan(values).any()
    thr, n_gt, n_eq, kept = sc.select_reference(values, k)
    assert n_gt < k <= n_gt + n_eq == len(kept)
    answer = sc.lv_key_inverse(np.sort(sc.lv_key(values))[-k:][:1])[0]
    assert answer == thr                     # (-0.0 == 0.0)
    if name.startswith('negative'):
        assert np.all(values < 0)
    if name.startswith('all_equal'):
        assert sc.decisive_pass(values, k) == 8 and n_eq == len(values)
    if name.startswith('minus_inf') and k > 60:
        assert thr == -np.inf and n_eq == 40


def test_further_pools_reach_the_zeros_and_the_denormals():
    hit = {float(sc.select_reference(v, k)[0])
           for name, v, k in _FURTHER if name.startswith('around_zero')}
    assert {0.0, 5e-324, -5e-324, 1e-323, -1e-323} <= hit
    both = [np.signbit(sc.lv_key_inverse(np.sort(sc.lv_key(v))[-k:][:1])[0])
            for name, v, k in _FURTHER
            if name.startswith('around_zero') and
            sc.select_reference(v, k)[0] == 0.0]
    assert True in both and False in both
    # the zeros and denormals are told apart in the last byte only
    assert any(sc.candidates_per_pass(v, k)[6] > 1
               for name, v, k in _FURTHER if name.startswith('around_zero'))


def test_select_reference_and_pools():
    for p in sc.SELECT_P:
        v = sc.random_pool(p)
        assert v.shape == (p,)
        for k in sc.select_ks(p):
            thr, n_gt, n_eq, kept = sc.select_reference(v, k)
            if k > p:
                assert thr == -np.inf and len(kept) == p
            else:
                assert n_gt < k <= n_gt + n_eq == len(kept)
        assert p < 30 or len(np.unique(v)) < p
    assert sc.select_ks(1) == [1, 2]
    assert sc.select_ks(5000) == [1, 2, 4999, 5000, 5001]
    for n in sc.APPEND_N:
        l = sc.live_batch(n, nan=True)
        assert np.isnan(l[0]) and np.isnan(l[-1])
    l = sc.live_batch(262145)
    assert np.sum(l == sc.LIVE_TIE) > 1000 and np.sum(l == -np.inf) > 1000
