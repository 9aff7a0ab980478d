"""pack_prior_table (nautilus_amd/csrc/nb_pack.h) on tables with the
closed-form kinds 7 to 17, built for the host by tests/pack_prior_check.cpp
the way tests/test_pack.py builds pack_check.cpp: the kernel level of every
mix of kinds, every value in the row the kernel reads (PT_LOC, PT_SCALE,
PT_P0 ... of nb_transform.hip), and every refusal.  The program is built a
second time with the address and undefined-behaviour sanitizers and must run
clean and print the same."""

import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.abspath(os.path.dirname(__file__)))
NPAR = 8                                 # NB_PRIOR_NPAR
OK, ERR_ARG, ERR_UNSUPPORTED = 0, 1, 3   # nb_common.h


def _build(tmp, name, extra):
    cxx = next((c for c in ('g++', 'c++', 'clang++', 'hipcc')
                if shutil.which(c)), None)
    assert cxx is not None, 'no C++ compiler (the build needs hipcc anyway)'
    exe = str(tmp / name)
    subprocess.check_call(
        [cxx, '-x', 'c++', '-std=c++17', '-O2'] + extra +
        ['-I', os.path.join(ROOT, 'nautilus_amd', 'csrc'),
         '-I', os.path.join(ROOT, 'include'),
         os.path.join(ROOT, 'tests', 'pack_prior_check.cpp'), '-o', exe])
    return exe


@pytest.fixture(scope='module')
def run(tmp_path_factory):
    """(index, images, the program's output) of the plain build"""
    tmp = tmp_path_factory.mktemp('pack_prior')
    out = subprocess.check_output([_build(tmp, 'plain', []), str(tmp)],
                                  text=True)
    index, images = {}, {}
    for line in out.splitlines():
        name, rc, level, nbytes, error = line.split('\t')
        assert name not in index
        index[name] = dict(rc=int(rc), level=int(level), error=error)
        img = np.fromfile(str(tmp / (name + '.bin')), dtype=np.uint8)
        assert img.size == int(nbytes)
        if int(rc) == OK:
            images[name] = img
    return index, images, out


def test_levels(run):
    level = {k: v['level'] for k, v in run[0].items() if v['rc'] == OK}
    assert level['level3_a'] == 3 and level['level3_b'] == 3
    assert level['level3_c'] == 3
    assert level['level4'] == 4 and level['level4_b'] == 4
    assert level['level5'] == 5 and level['level5_b'] == 5
    assert level['closed_13'] == 3 and level['closed_ends'] == 3
    # tables of the old kinds: what they always had (tests/test_pack.py)
    assert level['prior_level0'] == 0
    assert level['prior_8'] == 1 and level['prior_keys'] == 1
    assert level['prior_tails'] == 2
    assert len(level) == 13


def _split(img, d, n_keys):
    """par (NPAR, d), key_value, key_column, kind of an image"""
    assert img.size == (NPAR * d + n_keys) * 8 + 4 * n_keys + d
    par = img[:NPAR * d * 8].view(np.float64).reshape(NPAR, d)
    at = NPAR * d * 8
    key_value = img[at:at + 8 * n_keys].view(np.float64)
    at += 8 * n_keys
    key_column = img[at:at + 4 * n_keys].view(np.int32)
    return par, key_value, key_column, img[at + 4 * n_keys:]


def _rows(kinds, shape0):
    """what the kernel reads of columns of closed-form kinds, uniform and
    normal: loc, scale, then 1 / shape (13, 15, 16) or c and 1 - c (17)"""
    d = len(kinds)
    j = np.arange(d)
    want = np.zeros((NPAR, d))
    want[0], want[1] = 0.5 + j, 1.25 + j / 4.0
    for col, (kind, a) in enumerate(zip(kinds, shape0)):
        if kind in (13, 15, 16):
            want[2, col] = 1.0 / a
        elif kind == 17:
            want[2, col], want[3, col] = a, 1.0 - a
    return want


def test_every_value_sits_in_the_row_the_kernel_reads(run):
    kinds = [7, 8, 9, 10, 11, 12, 13, 14, 15, 16, 17, 13, 17]
    shape0 = [11.0 + j for j in range(13)]
    for j, a in [(6, 2.5), (8, 3.0), (9, 0.2), (10, 0.3), (11, 1.0),
                 (12, 1.0)]:
        shape0[j] = a
    par, key_value, key_column, kind = _split(run[1]['closed_13'], 13, 3)
    # bit for bit: the reciprocal is one IEEE division, 1 - c one subtraction
    assert np.array_equal(par.view(np.int64),
                          _rows(kinds, shape0).view(np.int64))
    assert par[2, 9] == 5.0 and par[3, 10] == 0.7 and par[3, 12] == 0.0
    assert list(kind) == kinds
    assert list(key_column) == [12, -1, 6]
    assert np.array_equal(key_value, [0.375, 1.375, 2.375])

    par, _, _, kind = _split(run[1]['closed_ends'], 3, 1)
    assert np.array_equal(par, _rows([17, 17, 13], [0.0, 1.0, 1e308]))
    assert par[2, 2] > 0 and list(par[2:4, 0]) == [0.0, 1.0]
    assert list(par[2:4, 1]) == [1.0, 0.0] and list(kind) == [17, 17, 13]

    for name, kinds, shape0 in [('level3_a', [0, 7], [11.0, 12.0]),
                                ('level4', [1, 8], [11.0, 12.0]),
                                ('level3_c', [17], [0.25])]:
        par, key_value, key_column, kind = _split(run[1][name], len(kinds), 1)
        assert np.array_equal(par, _rows(kinds, shape0)), name
        assert list(kind) == kinds and list(key_column) == [-1]
        assert key_value[0] == 0.375


def test_closed_form_columns_beside_the_old_kinds(run):
    """the rows of a closed-form column do not depend on its neighbours, and
    the neighbours keep theirs: log-uniform, log-normal, both truncnorms"""
    par, _, _, kind = _split(run[1]['level3_b'], 3, 1)
    assert list(kind) == [2, 9, 14]
    assert np.array_equal(par[:, 1:], _rows([2, 9, 14], [0, 0, 0])[:, 1:])
    assert abs(par[2, 0] - np.log(0.5)) < 1e-15
    assert abs(par[3, 0] - (np.log(8.0) - np.log(0.5))) < 1e-15
    assert not par[4:, 0].any()

    par, _, _, kind = _split(run[1]['level4_b'], 2, 1)
    assert list(kind) == [13, 3]
    assert np.array_equal(par[:, 0], _rows([13, 0], [2.5, 0])[:, 0])
    assert par[2, 1] == 0.75 and not par[3:, 1].any()

    par, _, _, kind = _split(run[1]['level5'], 2, 1)
    assert list(kind) == [6, 15]                 # rewritten from kind 5
    assert list(par[2:4, 0]) == [36.0, 40.0] and par[7, 0] == 1.0
    assert np.array_equal(par[:, 1], _rows([0, 15], [0, 3.0])[:, 1])
    # the same far interval as in a table of truncnorms alone
    alone = _split(run[1]['prior_tails'], 3, 1)[0]
    assert np.array_equal(par[2:, 0], alone[2:, 0])

    par, _, _, kind = _split(run[1]['level5_b'], 3, 1)
    assert list(kind) == [15, 6, 0]
    assert par[2, 0] == 2.0 and not par[3:, 0].any()
    assert list(par[2:4, 1]) == [38.0, np.inf] and par[7, 1] == -1.0
    assert not par[2:, 2].any()


def test_refusals(run):
    index = run[0]
    shape = {
        'weibull_zero': 'Weibull', 'weibull_negative': 'Weibull',
        'weibull_inf': 'Weibull', 'weibull_nan': 'Weibull',
        'weibull_tiny': 'Weibull', 'pareto_negative': 'Pareto',
        'pareto_zero': 'Pareto', 'pareto_inf': 'Pareto',
        'powerlaw_zero': 'power law', 'powerlaw_nan': 'power law',
        'powerlaw_inf': 'power law', 'triang_above': 'triangular',
        'triang_below': 'triangular', 'triang_nan': 'triangular',
        'triang_inf': 'triangular'}
    for name, family in shape.items():
        got = index[name]
        assert got['rc'] == ERR_ARG and got['level'] == -1, name
        assert got['error'].startswith('parameter 1: ' + family), got
    assert index['triang_above']['error'] == \
        'parameter 1: triangular needs a shape 0 <= c <= 1'
    assert index['pareto_negative']['error'] == \
        'parameter 1: Pareto needs a finite shape b > 0 with a finite ' \
        'reciprocal'
    for name in ('cauchy_scale', 'rayleigh_loc'):
        assert index[name]['rc'] == ERR_ARG
        assert index[name]['error'] == \
            'parameter 1: loc must be finite and scale positive'
    # kind 6 keeps the text that tests/golden/pack.npz recorded for it
    for name, kind in [('kind6', 6), ('kind6_after_closed', 6),
                       ('kind18', 18), ('kind255', 255)]:
        assert index[name]['rc'] == ERR_UNSUPPORTED, name
        assert index[name]['error'] == \
            'prior kind %d of parameter 1 is not supported' % kind
    refused = [k for k, v in index.items() if v['rc'] != OK]
    assert len(refused) == 21 and len(index) == 34


def test_sanitized_build_runs_clean(run, tmp_path):
    """host code with its own main: AddressSanitizer and UBSan, any report
    ends the program with a nonzero status"""
    exe = _build(tmp_path, 'sanitized',
                 ['-g', '-fsanitize=address,undefined',
                  '-fno-sanitize-recover=all'])
    done = subprocess.run([exe, str(tmp_path)], text=True,
                          stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert done.returncode == 0, done.stderr
    assert done.stderr == ''
    assert done.stdout == run[2]
