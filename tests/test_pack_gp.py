"""The packer of the Gaussian-process likelihood (``pack_gp`` of
nautilus_amd/csrc/nb_pack.h, all of ``nb_gp_create`` but the upload), built
for the host by tests/gp_pack_check.cpp.  The layout formulas of nb_layout.h
are written out again here in numpy, from the reading side: for every double
the kernel of nb_gp.hip reads, the distance that has to be there, and zeros in
the padding.  Every refusal returns its code and its message.  The same
program runs once more under the address and undefined-behaviour
sanitizers."""

import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.abspath(os.path.dirname(__file__)))
TILE = 256
SIZES = (1, 2, 16, 17, 37, 64, 127, 128)
ERR_ARG = 1

GENERAL = ('bad Gaussian-process likelihood arguments (n_data 1..128, data, '
           'a kernel NB_GP_SQEXP .. NB_GP_MATERN52, a finite log_norm)')
REFUSALS = {
    'gp_no_data_points': GENERAL, 'gp_too_many': GENERAL,
    'gp_kernel_below': GENERAL, 'gp_kernel_above': GENERAL,
    'gp_null_data': GENERAL, 'gp_null_out': GENERAL, 'gp_log_norm': GENERAL,
    'gp_data_inf': 'data point 3 must be finite',
    'gp_data_nan': 'data point 4 must be finite',
    'gp_sigma2_negative': 'sigma2 2 must be finite and not negative',
    'gp_sigma2_inf': 'sigma2 1 must be finite and not negative',
    'gp_dist_asymmetric': 'dist entry (3, 1) must be finite, not negative, '
                          'equal to entry (1, 3) and zero on the diagonal',
    'gp_dist_asymmetric_upper': 'dist entry (3, 1) must be finite, not '
                                'negative, equal to entry (1, 3) and zero on '
                                'the diagonal',
    'gp_dist_negative': 'dist entry (4, 2) must be finite, not negative, '
                        'equal to entry (2, 4) and zero on the diagonal',
    'gp_dist_inf': 'dist entry (4, 0) must be finite, not negative, equal to '
                   'entry (0, 4) and zero on the diagonal',
    'gp_dist_nan': 'dist entry (2, 1) must be finite, not negative, equal to '
                   'entry (1, 2) and zero on the diagonal',
    'gp_dist_diagonal': 'dist entry (3, 3) must be finite, not negative, '
                        'equal to entry (3, 3) and zero on the diagonal',
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
         os.path.join(ROOT, 'tests', 'gp_pack_check.cpp'), '-o', exe])
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
    return build(tmp_path_factory.mktemp('gp_pack'), 'gp_pack_check', ['-O2'])


@pytest.fixture(scope='module')
def packed(exe, tmp_path_factory):
    return run(exe, str(tmp_path_factory.mktemp('gp_pack_out')))


def inputs(p):
    """data, sigma2 and dist of gp_pack_check.cpp"""
    j = np.arange(p)
    hi, lo = np.maximum(j[:, None], j[None, :]), np.minimum(j[:, None],
                                                            j[None, :])
    dist = np.where(hi != lo, 1000.0 * hi + lo + 0.5, 0.0)
    return 3000000.0 + j, 0.5 + j, dist


def read_side(p, with_dist=True, with_sigma2=True):
    """The table as the kernel reads it (nb_gp.hip, the fill stage): d and
    sigma^2 at [0, 16 T) and [16 T, 32 T); then T (T + 1) / 2 tiles, number t
    being tile (ti, tj) with ti the largest integer whose ti (ti + 1) / 2 is
    at most t; double e of the region is row 16 ti + e % 16 and column 16 tj +
    (e / 16) % 16."""
    t_count = (p + 15) // 16
    data, sigma2, dist = inputs(p)
    head = np.zeros(32 * t_count)
    head[:p] = data
    if with_sigma2:
        head[16 * t_count:16 * t_count + p] = sigma2
    if not with_dist:
        return head
    e = np.arange(t_count * (t_count + 1) // 2 * TILE)
    t = e // TILE
    ti = ((np.sqrt(8 * t + 1) - 1) / 2).astype(int)
    assert np.all((ti * (ti + 1) // 2 <= t) & ((ti + 1) * (ti + 2) // 2 > t))
    tj = t - ti * (ti + 1) // 2
    row = 16 * ti + e % 16
    col = 16 * tj + (e // 16) % 16
    inside = (row < p) & (col <= row)
    tiles = np.where(inside, dist[np.minimum(row, p - 1),
                                  np.minimum(col, p - 1)], 0.0)
    return np.concatenate([head, tiles])


def test_cases(packed):
    index, images = packed
    want = {'gp_%d' % p for p in SIZES} | {
        'gp_37_no_dist', 'gp_37_no_sigma2', 'gp_5_first_kernel',
        'gp_5_last_kernel'}
    assert set(images) == want
    assert set(index) == want | set(REFUSALS)


@pytest.mark.parametrize('p', SIZES)
def test_every_distance_sits_where_the_kernel_reads_it(packed, p):
    img = packed[1]['gp_%d' % p]
    want = read_side(p)
    t_count = (p + 15) // 16
    assert img.size == 32 * t_count + t_count * (t_count + 1) // 2 * TILE
    assert np.array_equal(img, want)
    # every distance of the lower triangle, the diagonal's zeros aside, once
    _, _, dist = inputs(p)
    low = dist[np.tril_indices(p, -1)]
    tiles = img[32 * t_count:]
    assert np.array_equal(np.sort(tiles[tiles != 0.0]), np.sort(low))


def test_optional_inputs(packed):
    images = packed[1]
    assert np.array_equal(images['gp_37_no_dist'],
                          read_side(37, with_dist=False))
    assert images['gp_37_no_dist'].size == 32 * 3
    assert np.array_equal(images['gp_37_no_sigma2'],
                          read_side(37, with_sigma2=False))
    # the kernel is the handle's business, not the image's
    assert np.array_equal(images['gp_5_first_kernel'], read_side(5))
    assert np.array_equal(images['gp_5_last_kernel'], read_side(5))


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
    exe = build(tmp_path, 'gp_pack_check_san',
                ['-O1', '-g', '-fsanitize=address,undefined',
                 '-fno-sanitize-recover=all', '-fno-omit-frame-pointer'])
    index, images = run(exe, str(tmp_path / 'out'))
    assert index == packed[0]
    assert set(images) == set(packed[1])
    for name, img in images.items():
        assert np.array_equal(img, packed[1][name]), name
