"""The packer of the Gaussian-process likelihood of an ordered series
(``pack_gps`` of nautilus_amd/csrc/nb_pack.h, all of ``nb_gps_create`` but the
upload), built for the host by tests/gps_pack_check.cpp.  The layout of
nb_layout.h is written out again here in numpy, from the reading side: for
every double the filter of nb_gps_filter.h reads, the number that has to be
there.  Every refusal returns its code and its message.  The same program
runs once more under the address and undefined-behaviour sanitizers."""

import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.abspath(os.path.dirname(__file__)))
SIZES = (1, 2, 31, 32, 33, 65, 1000)
MOST = 1 << 20
ERR_ARG = 1

GENERAL = ('bad Gaussian-process series likelihood arguments (n_data '
           '1..1048576, t, data, a kernel NB_GPS_EXP .. NB_GPS_SHO, a finite '
           'log_norm)')
REFUSALS = {
    'gps_no_data_points': GENERAL, 'gps_too_many': GENERAL,
    'gps_kernel_below': GENERAL, 'gps_kernel_above': GENERAL,
    'gps_null_t': GENERAL, 'gps_null_data': GENERAL, 'gps_null_out': GENERAL,
    'gps_log_norm': GENERAL,
    'gps_t_inf_first': 't 0 must be finite',
    'gps_t_inf_last': 't 4 must be finite',
    'gps_t_nan': 't 2 must be finite',
    'gps_t_decreases': 't must not decrease: t 3 is below t 2',
    'gps_t_decreases_at_once': 't must not decrease: t 1 is below t 0',
    'gps_step_overflows': 't 2 is too far from t 1: the step is not finite',
    'gps_data_inf': 'data point 3 must be finite',
    'gps_data_nan': 'data point 4 must be finite',
    'gps_sigma2_negative': 'sigma2 2 must be finite and not negative',
    'gps_sigma2_inf': 'sigma2 1 must be finite and not negative',
}


def build(tmp, name, flags):
    cxx = next((c for c in ('g++', 'c++', 'clang++', 'hipcc')
                if shutil.which(c)), None)
    assert cxx is not None, 'no C++ compiler (the build needs hipcc anyway)'
    exe = str(tmp / name)
    subprocess.check_call(
        [cxx, '-x', 'c++', '-std=c++17', *flags,
         '-I', os.path.join(ROOT, 'nautilus_amd', 'csrc'),
         '-I', os.path.join(ROOT, 'include'),
         os.path.join(ROOT, 'tests', 'gps_pack_check.cpp'), '-o', exe])
    return exe


def run(exe, out_dir):
    """(index, images) of the program's run of every case"""
    os.makedirs(out_dir, exist_ok=True)
    out = subprocess.check_output([exe, out_dir], text=True)
    index, images = {}, {}
    for line in out.splitlines():
        name, rc, count, error = line.split('\t')
        assert name not in index
        index[name] = (int(rc), error)
        img = np.fromfile(os.path.join(out_dir, name + '.bin'))
        assert img.size == int(count)
        if int(rc) == 0:
            images[name] = img
    return index, images


@pytest.fixture(scope='module')
def exe(tmp_path_factory):
    return build(tmp_path_factory.mktemp('gps_pack'), 'gps_pack_check',
                 ['-O2'])


@pytest.fixture(scope='module')
def packed(exe, tmp_path_factory):
    return run(exe, str(tmp_path_factory.mktemp('gps_pack_out')))


def inputs(p):
    """t, data and sigma2 of gps_pack_check.cpp"""
    j = np.arange(p, dtype=float)
    return 0.5 * j * (j + 1.0) + 0.25, 3000000.0 + j, 0.5 + j


def read_side(p, t=None, with_sigma2=True):
    """The table as the kernel reads it (nb_gps_filter.h, the step loop): datum j
    at doubles 4 j .. 4 j + 3: the step t_j - t_j-1 (0 at j = 0), d_j,
    sigma_j^2 and a zero."""
    t0, data, sigma2 = inputs(p)
    t = t0 if t is None else t
    img = np.zeros((p, 4))
    img[1:, 0] = t[1:] - t[:-1]
    img[:, 1] = data
    if with_sigma2:
        img[:, 2] = sigma2
    return img.reshape(-1)


def test_cases(packed):
    index, images = packed
    want = {'gps_%d' % p for p in SIZES} | {
        'gps_37_no_sigma2', 'gps_5_first_kernel', 'gps_5_last_kernel',
        'gps_5_equal_times', 'gps_most'}
    assert set(images) == want
    assert set(index) == want | set(REFUSALS)


@pytest.mark.parametrize('p', SIZES + (MOST,))
def test_every_number_sits_where_the_kernel_reads_it(packed, p):
    img = packed[1]['gps_most' if p == MOST else 'gps_%d' % p]
    assert img.size == 4 * p
    assert np.array_equal(img, read_side(p))
    # the closed forms: step j is j, and no two entries of a datum agree
    assert np.array_equal(img[0::4], np.arange(p))


def test_optional_inputs(packed):
    images = packed[1]
    assert np.array_equal(images['gps_37_no_sigma2'],
                          read_side(37, with_sigma2=False))
    # the kernel is the handle's business, not the image's
    assert np.array_equal(images['gps_5_first_kernel'], read_side(5))
    assert np.array_equal(images['gps_5_last_kernel'], read_side(5))
    t = inputs(5)[0]
    t[2] = t[3] = t[1]
    want = read_side(5, t)
    assert want[8] == 0.0 and want[12] == 0.0 and want[16] > 0.0
    assert np.array_equal(images['gps_5_equal_times'], want)


def test_refusals(packed):
    index = packed[0]
    for name, message in REFUSALS.items():
        assert index[name] == (ERR_ARG, message), name
    for name in packed[1]:
        assert index[name] == (0, ''), name


def test_under_the_sanitizers(packed, tmp_path):
    """The same program, built with -fsanitize=address,undefined and run on
    its own: it gives the same lines and the same images, and neither
    sanitizer reports anything."""
    exe = build(tmp_path, 'gps_pack_check_san',
                ['-O1', '-g', '-fsanitize=address,undefined',
                 '-fno-sanitize-recover=all', '-fno-omit-frame-pointer'])
    index, images = run(exe, str(tmp_path / 'out'))
    assert index == packed[0]
    assert set(images) == set(packed[1])
    for name, img in images.items():
        assert np.array_equal(img, packed[1][name]), name
