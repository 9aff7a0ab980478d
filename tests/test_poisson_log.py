"""The float64 log of the Poisson kernel (``po_log``,
nautilus_amd/csrc/nb_poisson_log.h) built for the host from the very header
the kernel includes, with contraction off as in the kernel, against long
double."""

import os
import shutil
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_po_log_stays_within_one_ulp(tmp_path):
    """The arrangement (fdlibm's: f - (f^2/2 - s (f^2/2 + R)) with log 2 split
    in two) is built for an error below 1 ulp; the kernel's value budget
    (test_poisson_likelihood_gpu.py) counts on 2.  Measured: 0.85 ulp."""
    assert np.finfo(np.longdouble).eps < 1e-18      # the yardstick is wider
    cxx = next((c for c in ('g++', 'c++', 'clang++', 'hipcc')
                if shutil.which(c)), None)
    assert cxx is not None, 'no C++ compiler (the build needs hipcc anyway)'
    exe = str(tmp_path / 'poisson_log_check')
    subprocess.check_call(
        [cxx, '-x', 'c++', '-std=c++17', '-O2', '-ffp-contract=off',
         '-I', os.path.join(ROOT, 'nautilus_amd', 'csrc'),
         os.path.join(ROOT, 'tests', 'poisson_log_check.cpp'), '-o', exe])
    out = subprocess.check_output([exe, '500000'], text=True).split()
    worst, where = float(out[0]), float(out[1])
    print('po_log: largest error %.4f ulp, at x = %.17g' % (worst, where))
    assert worst <= 1.0
