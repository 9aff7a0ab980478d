"""The Box-Muller arithmetic of the proposal draw (``draw_log``,
``draw_sincos``, ``draw_normal_pair``, nautilus_amd/csrc/nb_draw.h) on the
device, word by word, against mpmath at 120 bits (draw_words.exact) -- and a
sweep over all 2^32 words.  The argument of every function is u = (w + 1/2) /
2^32 = (2 w + 1) / 2^33 for a 32-bit Philox word w, exact in mpmath.

The bounds are derived, not taken from the kernel:

``draw_log``, 1 ulp: the design bound of fdlibm's e_log.c, whose arrangement
  it is; what nb_draw.h claims; the bar tests/test_poisson_log.py sets for
  ``po_log``.
sine and cosine, 2 ulp: y = (4 u - q) * (pi / 2 rounded) carries at most 1.35 x
  2^-53 relative error: 0.5 ulp from rounding the product, 0.35 x 2^-53 from
  the rounded pi / 2 (1.5707963267948966 is 6.1e-17 below pi / 2, 0.35 x 2^-53
  of it).  The condition numbers |y cot y| and |y tan y| are at most 1 on |y|
  <= pi / 4, so at most 1.35 ulp of the result come from y (an ulp is at least
  2^-53 of its value).  0.5 ulp for the final rounding and less than 0.15 ulp
  for the roundings inside the polynomial term (fdlibm's k_sin.c / k_cos.c
  bound their own error by that once y is taken as exact): 2.0 ulp.
z0, z1, relative error 8 x 2^-53: the 1 ulp of the log is at most 2 x 2^-53
  relative and the square root halves it: 1; the square root rounds: 1 (the
  product with -2 is exact); the 2 ulp of the sine / cosine: at most 4; the
  product rounds: 1.  7 x 2^-53 and terms of second order.
"""

import time

import numpy as np
import pytest

from draw_words import (corner_words, exact, NAMES, LOG_ULP, SINCOS_ULP,
                        PAIR_REL)

pytestmark = pytest.mark.gpu

N_RANDOM = 50000
CHUNK = 2**20          # words per chunk of the sweep: 4096 chunks


@pytest.fixture(scope='module')
def dev():
    import torch
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    from nautilus_amd import device
    return device


def check(dev, w0, w1, label):
    """Run the words through nb_draw_words and hold every value against the
    exact one; prints the worst case of every function."""
    ref = exact(w0, w1)
    got = dev.draw_words(w0, w1).cpu().numpy()
    worst = {}
    for j, name in enumerate(NAMES):
        hi, lo, ulp = ref[name]
        assert np.all(np.isfinite(got[:, j])), name
        err = np.abs(((got[:, j] - hi) - lo) / ulp)
        if name in ('z0', 'z1'):
            err = err * ulp / np.abs(hi) * 2.0**53
        i = int(np.argmax(err))
        worst[name] = float(err[i])
        print('%s %-3s largest error %.4f %s at w0 = 0x%08x, w1 = 0x%08x' % (
            label, name, err[i], 'x 2^-53' if name[0] == 'z' else 'ulp',
            w0[i], w1[i]))
    assert np.all(got[:, 0] < 0)
    assert np.all(np.abs(got[:, 1:3]) <= 1)
    assert worst['log'] <= LOG_ULP
    assert worst['sin'] <= SINCOS_ULP and worst['cos'] <= SINCOS_ULP
    assert worst['z0'] * 2.0**-53 <= PAIR_REL
    assert worst['z1'] * 2.0**-53 <= PAIR_REL
    return worst


def test_corner_words_against_mpmath(dev):
    """Every corner word of draw_words.py as the word of the log and as the
    word of the sine / cosine: 68131 rows, 1 to 3 s of mpmath.  Measured on
    the MI355X: log 0.73 ulp, sin 1.80 ulp at 0x75c646d6, cos 1.81 ulp at
    0xca33c991 (the two worst words of the host model), z0, z1 3.7 x 2^-53."""
    c = corner_words()
    t0 = time.time()
    check(dev, c, np.roll(c, -(len(c) // 2 + 1)), 'corner words:')
    print('%d rows in %.1f s' % (len(c), time.time() - t0))


def test_random_words_against_mpmath(dev):
    """N_RANDOM = 50000 fixed-seed random pairs of words: 0.6 to 2.5 s of
    mpmath.  Measured on the MI355X: log 0.73 ulp, sin 1.72 ulp, cos 1.77 ulp,
    z0, z1 3.5 x 2^-53."""
    r = np.random.default_rng(1).integers(0, 2**32, size=(N_RANDOM, 2),
                                          dtype=np.uint64).astype(np.uint32)
    t0 = time.time()
    check(dev, r[:, 0].copy(), r[:, 1].copy(), 'random words:')
    print('%d rows in %.1f s' % (N_RANDOM, time.time() - t0))


@pytest.fixture(scope='module')
def full_sweep(dev):
    import torch
    dev.draw_sweep(0, 4096, 4096)                # (loads the code object)
    torch.cuda.synchronize()
    t0 = time.time()
    out = dev.draw_sweep(0, 2**32, CHUNK)
    print('sweep of 2^32 words: %.2f s' % (time.time() - t0))
    return out


def test_sweep_of_every_word(dev, full_sweep):
    """nb_draw_sweep over all 2^32 words.  That no word gives a non-finite or
    out-of-range value (log >= 0, |sin| > 1, |cos| > 1) is proved for every
    word.  The ulp bounds are NOT: the sweep measures the difference from the
    device library's log / sincospi, which has an error of its own; it directs
    the exact check to the likely worst words -- the worst word of each of the
    64 chunks (of 2^20 words) with the largest difference, per function -- and
    these pass the bounds of this file against mpmath.  The largest difference
    from the library is printed, not asserted on.  Measured on the MI355X: the
    sweep takes 0.04 s; largest differences 1, 2 and 2 ulp; worst of the
    directed words against mpmath: log 0.53 ulp, sin 1.79 ulp, cos 1.82 ulp at
    0xc28c48da -- above anything the corner and the random words find."""
    bad, diff, word = full_sweep
    assert diff.shape == (3, 2**32 // CHUNK)
    assert bad.tolist() == [0, 0, 0]
    assert np.all(np.isfinite(diff))
    # every chunk reported a word of its own
    assert np.array_equal(word // CHUNK, np.tile(np.arange(diff.shape[1]),
                                                 (3, 1)))
    top = np.argsort(diff, axis=1)[:, -64:]
    for f, name in enumerate(NAMES[:3]):
        i = top[f, -1]
        print('%s: largest difference from the library %.4f ulp at 0x%08x' % (
            name, diff[f, i], word[f, i]))
    w_log = word[0, top[0]]
    w_trig = np.concatenate([word[1, top[1]], word[2, top[2]]])
    check(dev, np.tile(w_log, 2), w_trig, 'worst of the sweep:')


def test_sweep_ragged_ranges(dev, full_sweep):
    """Sweeps that start and end inside a chunk, inside a 4096-word tile and
    inside a wavefront's 64 words report, on the chunks they cover completely,
    exactly what the full sweep reports, and on the others a word of their
    range with a difference no larger; a sweep of one word reports that word;
    the last words up to 2^32 - 1 are their own range."""
    _, diff, word = full_sweep
    for first, count in ((3 * 2**29 - 2 * CHUNK - 12345, 4 * CHUNK + 777),
                         (2**32 - 1000, 1000), (5 * CHUNK + 63, 2),
                         (7 * CHUNK, CHUNK)):
        bad, d, w = dev.draw_sweep(first, count, CHUNK)
        assert bad.tolist() == [0, 0, 0]
        c0 = first // CHUNK
        assert d.shape == (3, (first + count - 1) // CHUNK - c0 + 1)
        assert np.all((w >= first) & (w.astype(np.int64) < first + count))
        for c in range(d.shape[1]):
            lo, hi = (c0 + c) * CHUNK, (c0 + c + 1) * CHUNK
            dc, wc, df, wf = d[:, c], w[:, c], diff[:, c0 + c], word[:, c0 + c]
            assert np.all(wc // CHUNK == c0 + c)
            if first <= lo and hi <= first + count:
                assert np.array_equal(dc, df) and np.array_equal(wc, wf)
            else:
                assert np.all((dc < df) | ((dc == df) & (wc <= wf)))
    # one word: the worst word of a chunk on its own gives the chunk's entry
    for f in range(3):
        wf = int(word[f, 1234])
        _, d, w = dev.draw_sweep(wf, 1, CHUNK)
        assert w[f, 0] == wf and d[f, 0] == diff[f, 1234]
    from nautilus_amd import _lib
    for args in ((0, 2**32 + 1, CHUNK), (2**32 - 5, 6, CHUNK), (0, 4096, 0),
                 (0, 4096, 4097), (0, 2**32, 4096)):
        with pytest.raises(_lib.NativeError) as err:
            dev.draw_sweep(*args)
        assert err.value.code == _lib.ERR_ARG
