"""The 32-bit words at which the Box-Muller arithmetic of the proposal draw
(nautilus_amd/csrc/nb_draw.h) can go wrong first, shared by the host model
test and the device test (tests/draw_words_check.cpp writes them out again in
C++).  The argument of every function is u = (w + 1/2) / 2^32."""

import numpy as np

# the worst words of the host model over 2 x 10^7 random words (sine, cosine)
MODEL_WORST = (0x75c646d6, 0xca33c991)

# error bounds, derived in tests/test_draw_words_gpu.py
LOG_ULP, SINCOS_ULP, PAIR_REL = 1.0, 2.0, 8.0 * 2.0**-53

PREC = 120             # bits of the mpmath reference
NAMES = ('log', 'sin', 'cos', 'z0', 'z1')


def corner_words():
    """Sorted, without repeats:
      0 .. 4095 and 2^32 - 1 - k, k < 4096         the ends of the range
      q 2^29 + k, q 2^29 - 1 - k, q = 1..7         where rint(4 u) changes (odd
                                                   q) and where its remainder
                                                   changes sign (even q)
      2^k, 2^k - 1                                 every binade of u
      64 words either side of sqrt(1/2) 2^(32-k)   where draw_log doubles its
                                                   mantissa
      MODEL_WORST"""
    k = np.arange(4096, dtype=np.int64)
    parts = [k, 2**32 - 1 - k]
    for q in range(1, 8):
        parts += [q * 2**29 + k, q * 2**29 - 1 - k]
    j = np.arange(-63, 65, dtype=np.int64)
    for e in range(32):
        parts += [np.array([2**e, 2**e - 1], dtype=np.int64),
                  int(np.floor(np.ldexp(np.sqrt(0.5), 32 - e))) + j]
    parts.append(np.array(MODEL_WORST, dtype=np.int64))
    w = np.unique(np.concatenate(parts))
    return w[(w >= 0) & (w < 2**32)].astype(np.uint32)


def exact(w0, w1):
    """log u(w0), sin 2 pi u(w1), cos 2 pi u(w1), sqrt(-2 log u(w0)) (cos, sin)
    2 pi u(w1) to PREC bits, each as (hi, lo, ulp): hi the leading 53 bits, lo
    the next 40 (both exact doubles), ulp = 2^(exponent - 52) of the value.
    (mpmath's internal functions on its raw numbers: a third of the time of the
    mpf class.)"""
    from mpmath.libmp import (from_man_exp, mpf_log, mpf_cos_sin_pi, mpf_sqrt,
                              mpf_mul, mpf_neg, mpf_shift)
    cols = [([], [], []) for _ in NAMES]
    for a, b in zip(w0.tolist(), w1.tolist()):
        lg = mpf_log(from_man_exp(2 * a + 1, -33), PREC, 'n')
        cs, sn = mpf_cos_sin_pi(from_man_exp(2 * b + 1, -32), PREC, 'n')
        r = mpf_sqrt(mpf_shift(mpf_neg(lg), 1), PREC, 'n')
        for col, v in zip(cols, (lg, sn, cs, mpf_mul(r, cs, PREC, 'n'),
                                 mpf_mul(r, sn, PREC, 'n'))):
            sign, man, exp, bc = v
            m = man >> (bc - 93) if bc >= 93 else man << (93 - bc)
            s = -1 if sign else 1
            col[0].append(s * (m >> 40))
            col[1].append(s * (m & 0xffffffffff))
            col[2].append(exp + bc - 1)
    out = {}
    for name, (hi, lo, e) in zip(NAMES, cols):
        e = np.array(e, dtype=np.int64)
        out[name] = (np.ldexp(np.array(hi, dtype=np.float64), e - 52),
                     np.ldexp(np.array(lo, dtype=np.float64), e - 92),
                     np.ldexp(1.0, e - 52))
    return out
