"""The Box-Muller arithmetic of the proposal draw (``draw_log``,
``draw_sincos``, ``draw_normal_pair``, nautilus_amd/csrc/nb_draw.h) built for
the host from the very header the kernels include, with contraction off,
against long double with the exact remainder of 4 u.

This is a MODEL of the device arithmetic: the reciprocal estimate that starts
the division of ``draw_log`` is a float-rounded 1 / b here, not the table of
the hardware, ``frexp`` is the C library's, and the device compiler may
contract a product and a sum that the host keeps apart.  The verdict on the
device is tests/test_draw_words_gpu.py."""

import os
import shutil
import subprocess

import numpy as np

from draw_words import (corner_words, exact, NAMES, PREC, LOG_ULP, SINCOS_ULP,
                        PAIR_REL)

ROOT = os.path.dirname(os.path.abspath(os.path.dirname(__file__)))


def test_draw_words_host_model(tmp_path):
    """The corner words of draw_words.py (every one as the word of the log and
    as the word of the sine / cosine) and 2 x 10^6 random pairs; the bounds
    are those of the device test, where they are derived.  Measured: log 0.78
    ulp, sine 1.80 ulp at 0x75c646d6, cosine 1.81 ulp at 0xca33c991, pair
    4.2 x 2^-53; over 2 x 10^7 pairs 0.81 / 1.81 / 1.81 ulp and 4.3 x 2^-53.
    One second."""
    assert np.finfo(np.longdouble).eps < 1e-18      # the yardstick is wider
    cxx = next((c for c in ('g++', 'c++', 'clang++', 'hipcc')
                if shutil.which(c)), None)
    assert cxx is not None, 'no C++ compiler (the build needs hipcc anyway)'
    exe = str(tmp_path / 'draw_words_check')
    subprocess.check_call(
        [cxx, '-x', 'c++', '-std=c++17', '-O2', '-ffp-contract=off',
         '-I', os.path.join(ROOT, 'nautilus_amd', 'csrc'),
         os.path.join(ROOT, 'tests', 'draw_words_check.cpp'), '-o', exe])
    out = subprocess.check_output([exe, '2000000'], text=True)
    rows = {r.split()[0]: r.split()[1:] for r in out.splitlines()}
    for name in ('log', 'sin', 'cos', 'pair'):
        print('%-4s largest error %s %s at %s' % (
            name, rows[name][0], 'x 2^-53' if name == 'pair' else 'ulp',
            rows[name][1]))
    # the program's list of corner words is the one the device test uses
    assert int(rows['corners'][0]) == len(corner_words())
    for name in ('log', 'sin', 'cos', 'pair'):
        assert int(rows[name][2]) == 0, name   # finite, log < 0, |sin| <= 1
    assert float(rows['log'][0]) <= LOG_ULP
    assert float(rows['sin'][0]) <= SINCOS_ULP
    assert float(rows['cos'][0]) <= SINCOS_ULP
    assert float(rows['pair'][0]) * 2.0**-53 <= PAIR_REL


def test_exact_reference_is_right():
    """The fast path into mpmath gives what its documented functions give at
    twice the precision (it is the yardstick of tests/test_draw_words_gpu.py)."""
    import mpmath
    w = np.array([0, 1, 2**29 - 1, 2**29, 0x75c646d6, 0xca33c991, 2**31,
                  3037000499, 2**32 - 1], dtype=np.uint32)
    ref = exact(w, w[::-1].copy())
    with mpmath.workprec(2 * PREC):
        for i, (a, b) in enumerate(zip(w.tolist(), w[::-1].tolist())):
            u0 = mpmath.mpf(2 * a + 1) / 2**33
            t = 2 * mpmath.pi * mpmath.mpf(2 * b + 1) / 2**33
            r = mpmath.sqrt(-2 * mpmath.log(u0))
            want = (mpmath.log(u0), mpmath.sin(t), mpmath.cos(t),
                    r * mpmath.cos(t), r * mpmath.sin(t))
            for name, v in zip(NAMES, want):
                hi, lo, ulp = ref[name]
                d = (v - mpmath.mpf(float(hi[i]))) - mpmath.mpf(float(lo[i]))
                assert abs(d) < float(ulp[i]) * 2.0**-39, (name, a, b)
                assert float(ulp[i]) <= abs(v) < 2 * float(ulp[i]) * 2.0**52
