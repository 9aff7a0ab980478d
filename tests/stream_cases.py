"""Cases and references of the kernel-level tests of stream compaction
(``nb_compact_rows``), shell statistics (``nb_shell_stats``) and the live pool
(``nb_live_append`` / ``nb_live_select`` / ``nb_live_stats``).  Plain numpy,
no device: shared by test_stream_cases.py (the references against independent
arithmetic and the radix pools against their claim, on the CPU) and
test_stream_ops_gpu.py (the kernels against these references).

The sizes are the edges of the kernels: 64 lanes of a wavefront, 256 threads
of a workgroup, ``CHUNK`` = 2048 flags per workgroup of the compaction, 256
chunks per round of its scan (``SCAN_ROWS`` = 524 288 rows), the 1024 x 256
grid cap of the shell statistics (grid stride from 262 144 values on) and the
1024 threads of the live-pool kernels."""

import functools
import math

import numpy as np

CHUNK = 2048
SCAN_ROWS = 256 * CHUNK

# ---------------------------------------------------------------------------
# stream compaction
# ---------------------------------------------------------------------------
COMPACT_SMALL_N = (1, 255, 256, 257, 2047, 2048, 2049)
COMPACT_SMALL_DIMS = (1, 2, 3, 7, 16, 50, 127, 128)
COMPACT_LARGE_N = (SCAN_ROWS - 1, SCAN_ROWS, SCAN_ROWS + 1,
                   2 * SCAN_ROWS + CHUNK + 1)
COMPACT_LARGE_DIMS = (1, 3)
# (mask, flip); (2, 2) is the call of the sampler's shell-exclusion loop
MASK_FLIP = ((1, 0), (2, 0), (2, 2), (1, 1), (3, 0), (0x80, 0), (0xff, 0x55))

# a flag byte that survives under every mask and flip once it is flipped, and
# has bit 0 set then: what the bytes behind the first n flags are filled with
def beyond_byte(flip):
    return 0xff ^ flip


def survivor_rows(n):
    """The rows of the single-survivor patterns that lie below n: both ends,
    either side of a wavefront, a round of 256 flags and a chunk, and the
    start of the last chunk's worth of rows."""
    rows = []
    for r in (0, n - 1, 63, 64, 255, 256, 2047, 2048, n - 2048):
        if 0 <= r < n and r not in rows:
            rows.append(r)
    return rows


def _seed(*words):
    return np.random.default_rng([20240611] + [int(w) for w in words])


def _frozen(a):
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=8)
def keep_patterns(n, large=False):
    """[(name, keep)]: which rows survive (read-only arrays).  ``large``
    leaves out the alternating pattern and one of the two random ones."""
    out = [('all_clear', np.zeros(n, dtype=bool)),
           ('all_set', np.ones(n, dtype=bool))]
    for r in survivor_rows(n):
        keep = np.zeros(n, dtype=bool)
        keep[r] = True
        out.append(('only_row_%d' % r, keep))
    if not large:
        out.append(('alternating', np.arange(n) % 2 == 1))
        out.append(('random_p0.01', _seed(n, 1).random(n) < 0.01))
    out.append(('random_p0.5', _seed(n, 2).random(n) < 0.5))
    return tuple((name, _frozen(keep)) for name, keep in out)


@functools.lru_cache(maxsize=8)
def noise_bytes(n):
    """Random bytes over the full range 0..255, read-only (every value occurs
    from n = 2047 on; asserted in test_stream_cases.py)."""
    return _frozen(_seed(n, 3).integers(0, 256, size=n, dtype=np.uint8))


def flags_for(keep, mask, flip, noise):
    """Flag bytes with ((flags ^ flip) & mask) != 0 exactly on ``keep``.  The
    bits outside the mask come from ``noise``; inside it a kept row carries
    the noise bits too, or the lowest bit of the mask if those are all
    clear.  So bit 0 is unrelated to the decision unless the mask holds it,
    and a mask of several bits sees every non-zero combination."""
    mask, flip = np.uint8(mask), np.uint8(flip)
    low = np.uint8(int(mask) & -int(mask))
    inside = noise & mask
    inside = np.where(inside == 0, low, inside)
    plain = (noise & ~mask) | np.where(keep, inside, np.uint8(0))
    return (plain ^ flip).astype(np.uint8)


def flag_patterns(n, mask, flip, large=False):
    """[(name, flags)]: ``keep_patterns`` as flag bytes for (mask, flip), and
    the raw ``noise_bytes`` whose survivors follow from the mask alone."""
    noise = noise_bytes(n)
    out = [(name, flags_for(keep, mask, flip, noise))
           for name, keep in keep_patterns(n, large)]
    out.append(('bytes', noise.copy()))
    return out


def compact_reference(x, flags, mask, flip):
    """(rows, src_idx, counts) of include/nautilus_hip.h: the rows of ``x``
    with ((flags ^ flip) & mask) != 0 in input order, their source rows,
    counts[0] = rows with bit 0 of flags ^ flip set, counts[1] = rows kept."""
    f = np.asarray(flags, dtype=np.uint8) ^ np.uint8(flip)
    src_idx = np.flatnonzero((f & np.uint8(mask)) != 0).astype(np.int64)
    counts = np.array([np.count_nonzero(f & np.uint8(1)), len(src_idx)],
                      dtype=np.int64)
    return np.asarray(x)[src_idx], src_idx, counts


def compact_points(n, n_dim):
    """Rows to compact: Gaussian values with -0.0, a denormal, +-inf and a
    NaN among them (the kernels copy bits)."""
    x = _seed(n, n_dim, 4).standard_normal((n, n_dim))
    flat = x.reshape(-1)
    special = (-0.0, 5e-324, np.inf, -np.inf, np.nan)
    for i, v in enumerate(special):
        flat[(i * 7919) % flat.size] = v
    return x


# ---------------------------------------------------------------------------
# shell statistics
# ---------------------------------------------------------------------------
LSE_N = (1, 63, 64, 65, 255, 256, 257, 262143, 262144, 262145, 524289)
LSE_RTOL = LSE_ATOL = 1e-13        # test_hip_parity.test_shell_stats_match_reference


def _logsumexp_ld(l):
    """logsumexp in long double: maximum subtracted, terms and sum in
    np.longdouble (numpy sums pairwise)."""
    l = np.asarray(l, dtype=np.float64)
    if l.size == 0:
        return -np.inf
    if np.isnan(l).any():
        return np.nan
    m = l.max()
    if np.isinf(m):
        return float(m)
    terms = np.exp(l.astype(np.longdouble) - np.longdouble(m))
    return float(np.longdouble(m) + np.log(np.sum(terms)))


def lse_reference(l, threshold):
    """(logsumexp(l), logsumexp(2 l), max l, #(l >= threshold)); -inf for an
    empty or all -inf input."""
    l = np.asarray(l, dtype=np.float64)
    if l.size == 0:
        return -np.inf, -np.inf, -np.inf, 0
    return (_logsumexp_ld(l), _logsumexp_ld(2.0 * l), float(l.max()),
            int(np.count_nonzero(l >= threshold)))


def live_stats_reference(l, thr):
    """(#(l > thr), logsumexp(l | l > thr), #(l == thr))."""
    l = np.asarray(l, dtype=np.float64)
    return (int(np.count_nonzero(l > thr)), _logsumexp_ld(l[l > thr]),
            int(np.count_nonzero(l == thr)))


def tail_block_start(n):
    """First index of the last, possibly partial, block of 256."""
    return (n - 1) // 256 * 256


def lse_contents(n):
    """[(name, values, tie)]: ``tie`` is a value of the input, one that
    occurs several times wherever the content allows it (not in the strictly
    monotone ones and not at n = 1)."""
    def lone(at, value):
        l = np.full(n, -np.inf)
        l[at] = value
        return l

    rng = _seed(n, 5)
    i = np.arange(n, dtype=np.float64)
    out = [('all_equal', np.full(n, -3.7), -3.7),
           ('finite_first', lone(0, 2.5), 2.5),
           ('finite_last', lone(n - 1, -812.25), -812.25),
           ('finite_at_63', lone(min(63, n - 1), 0.125), 0.125),
           ('finite_tail_block', lone(tail_block_start(n), 41.0), 41.0)]
    l = rng.standard_normal(n) * 3
    l[:: max(1, n // 5)] = l[0]
    l[n - 1] = l.max() + 1.75
    out.append(('max_last', l, l[0] if n > 1 else l[n - 1]))
    # (steps of 2^-10: exact, so strictly monotone at every n)
    out.append(('ascending', i / 1024 - 300.0, (n // 2) / 1024 - 300.0))
    out.append(('descending', 700.0 - i / 1024, 700.0 - (n // 3) / 1024))
    l = rng.uniform(-1500.0, 0.0, n)
    l[:: max(1, n // 7)] = l[n // 2]
    out.append(('wide_range', l, l[n // 2]))
    l = rng.standard_normal(n) * 30
    l[rng.permutation(n)[:n // 2]] = -np.inf
    l[n // 2] = 11.5
    l[:: max(1, n // 3)] = 11.5
    out.append(('half_minus_inf', l, 11.5))
    return out


def between(l):
    """A threshold that is no input value: halfway between the two middle
    distinct finite values, or just below the only one."""
    u = np.unique(l[np.isfinite(l)])
    if len(u) < 2:
        return float(np.nextafter(u[0], -np.inf))
    a, b = u[len(u) // 2 - 1], u[len(u) // 2]
    mid = a + (b - a) / 2
    assert a < mid < b
    return float(mid)


def lse_thresholds(l, tie):
    return [('minus_inf', -np.inf), ('plus_inf', np.inf), ('tie', float(tie)),
            ('between', between(l))]


def nonfinite_positions(n):
    """Where the single NaN / +inf element is planted."""
    return sorted({0, min(63, n - 1), n // 2, tail_block_start(n), n - 1})


# ---------------------------------------------------------------------------
# live pool: the order-preserving key of the radix selection
# ---------------------------------------------------------------------------
_SIGN = np.uint64(1 << 63)


def lv_key(v):
    """nb_live.hip's lv_key: double -> uint64, ascending with the value."""
    b = np.ascontiguousarray(v, dtype=np.float64).view(np.uint64)
    return np.where(b >> np.uint64(63) != 0, ~b, b | _SIGN)


def lv_key_inverse(key):
    key = np.ascontiguousarray(key, dtype=np.uint64)
    bits = np.where(key >> np.uint64(63) != 0, key & ~_SIGN, ~key)
    return np.ascontiguousarray(bits).view(np.float64)


def kth_largest(values, k):
    return np.sort(np.asarray(values, dtype=np.float64))[-k]


def candidates_per_pass(values, k):
    """For the k-th largest KEY of the pool: how many keys share its top
    8 (i + 1) bits, i = 0..7 -- the candidates the selection still has after
    pass i."""
    keys = lv_key(values)
    answer = np.sort(keys)[-k]
    return [int(np.count_nonzero(keys >> np.uint64(56 - 8 * i) ==
                                 answer >> np.uint64(56 - 8 * i)))
            for i in range(8)]


def decisive_pass(values, k):
    """The first pass after which one candidate is left (8 if never: ties)."""
    left = candidates_per_pass(values, k)
    return next((i for i, c in enumerate(left) if c == 1), 8)


RADIX_P = 200


def _radix_pool(j, top):
    """RADIX_P keys that share their top j bytes (the first is ``top``) and
    all differ in byte j, which takes 0 and 255 among its values; random
    bytes below.  j = 0: the top bytes themselves differ, over both signs
    (0x01..0xfe: neither a NaN nor an infinity)."""
    rng = _seed(j, top, 6)
    if j == 0:
        digit = np.concatenate([[0x01, 0xfe],
                                2 + rng.permutation(252)[:RADIX_P - 2]])
    else:
        digit = np.concatenate([[0, 255],
                                1 + rng.permutation(254)[:RADIX_P - 2]])
    assert len(np.unique(digit)) == RADIX_P
    keys = np.zeros(RADIX_P, dtype=np.uint64)
    if j > 0:
        prefix = [top] + [int(b) for b in rng.integers(0, 256, j - 1)]
        for b in prefix:
            keys = (keys << np.uint64(8)) | np.uint64(b)
    keys = (keys << np.uint64(8)) | digit.astype(np.uint64)
    for _ in range(7 - j):
        keys = (keys << np.uint64(8)) | rng.integers(
            0, 256, RADIX_P).astype(np.uint64)
    return lv_key_inverse(rng.permutation(keys))


def radix_cases():
    """[(name, values, k, pass)]: the k-th largest of ``values`` is decided
    in pass ``pass`` of the selection and no earlier.  Per decisive byte one
    pool of negative and one of positive values (j = 0: one pool over both),
    each with k = 77, k = 1 (the key whose byte is 255) and k = p (the key
    whose byte is 0)."""
    out = []
    for j in range(8):
        for sign, top in (('neg', 0x40), ('pos', 0xbf)):
            if j == 0 and sign == 'pos':
                continue
            v = _radix_pool(j, top)
            for k in (77, 1, RADIX_P):
                out.append(('byte%d_%s_k%d' % (j, 'mixed' if j == 0 else sign,
                                               k), v, k, j))
    return out


def further_pools():
    """[(name, values, k)]: negative values only; values straddling zero
    with both zeros and the smallest denormals of both signs; -inf among
    finite values; p equal values."""
    rng = _seed(7)
    tiny = 5e-324
    neg = -np.exp(rng.uniform(-700, 700, 300))
    zero = np.array([-1.0, -2.5e-308, -2 * tiny, -tiny, -0.0, 0.0, tiny,
                     2 * tiny, 2.5e-308, 1.0, -0.0, 0.0])
    ninf = np.concatenate([np.full(40, -np.inf), rng.standard_normal(60)])
    rng.shuffle(ninf)
    equal = np.full(333, -17.25)
    out = []
    for name, v, ks in (('negative', neg, (1, 150, 300)),
                        ('around_zero', zero, tuple(range(1, 13))),
                        ('minus_inf_mixed', ninf, (1, 60, 61, 100)),
                        ('all_equal', equal, (1, 200, 333))):
        out += [('%s_k%d' % (name, k), v, k) for k in ks]
    return out


def select_reference(values, k):
    """(threshold, #above, #equal, kept values sorted) of nb_live_select:
    the k-th largest value, or -inf and everything kept with fewer than k."""
    v = np.asarray(values, dtype=np.float64)
    thr = kth_largest(v, k) if len(v) >= k else -np.inf
    return (float(thr), int(np.count_nonzero(v > thr)),
            int(np.count_nonzero(v == thr)), np.sort(v[v >= thr]))


SELECT_P = (1, 255, 256, 1023, 1024, 1025, 5000)


def select_ks(p):
    """k = 1, 2, p - 1, p, p + 1 (those that are at least 1)."""
    return sorted({k for k in (1, 2, p - 1, p, p + 1) if k >= 1})


def random_pool(p):
    """Gaussian values, a tenth of them tied in threes."""
    v = _seed(p, 8).standard_normal(p) * 5
    t = p // 30
    v[t:2 * t] = v[:t]
    v[2 * t:3 * t] = v[:t]
    return v


APPEND_N = (1, 256, 262144, 262145)
STATS_N = (0, 1, 1023, 1024, 1025, 70001)
LIVE_ATOL = 1e-12                              # test_live_gpu.py
LIVE_TIE = 0.75


def live_batch(n, nan=False):
    """A batch of log L: Gaussian, a fifth -inf, every ninth value tied at
    ``LIVE_TIE``, optionally NaNs at both ends and in the middle."""
    rng = _seed(n, 9)
    l = rng.standard_normal(n) * 4
    l[rng.random(n) < 0.2] = -np.inf
    l[4::9] = LIVE_TIE
    if nan:
        l[[0, n // 2, n - 1]] = np.nan
    return l


def fsum_logsumexp(l):
    """logsumexp with an exactly rounded sum of the double terms (math.fsum):
    a second opinion on the long double sum for benign input."""
    l = np.asarray(l, dtype=np.float64)
    m = l.max()
    return m + math.log(math.fsum(np.exp(l - m).tolist()))
