"""The argument checks and the slot plan of the Gaussian-process series
likelihood (``plan_gps_terms`` of nautilus_amd/csrc/nb_pack.h for a sum of
terms, all of ``nb_gps_create_terms`` but ``pack_gps`` and the upload, and
``plan_gps_one`` for one term), built for the host by
tests/gps_terms_check.cpp.  The plan is written out again here from the
reading side -- where the filter of nb_gps_filter.h finds every slot -- for
each of the four kernels alone and for every sequence of two or three kernel
codes; every refusal returns its code and its own message.  The same program
runs once more under the address and undefined-behaviour sanitizers."""

import itertools
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.abspath(os.path.dirname(__file__)))
ERR_ARG = 1
STATES = (1, 2, 3, 2)                  # exp, matern32, matern52, sho
COLUMNS = (2, 2, 2, 3)                 # (a, l) or (a, l, q)

TOO_MANY = ('the terms of the Gaussian-process series likelihood have %d '
            'states (exp 1, matern32 2, matern52 3, sho 2): at most 6, in at '
            'most 3 terms')
COUNT = ('the Gaussian-process series likelihood of a sum takes 2..3 terms, '
         'not %d (one term goes through nb_gps_create)')
CODE = ('term %d of the Gaussian-process series likelihood has kernel %d: '
        'not one of NB_GPS_EXP .. NB_GPS_SHO')
NULL = ('the Gaussian-process series likelihood of a sum of terms needs '
        'kernels, t, data and out: no NULL pointer')
REFUSALS = {
    'no_terms': COUNT % 0, 'one_term': COUNT % 1, 'four_terms': COUNT % 4,
    'negative_terms': COUNT % -2,
    'code_above': CODE % (0, 4), 'code_below': CODE % (2, -1),
    'two_bad_codes': CODE % (1, 7),
    'null_kernels': NULL, 'null_t': NULL, 'null_data': NULL, 'null_out': NULL,
    'null_out_one_term': NULL,
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
         os.path.join(ROOT, 'tests', 'gps_terms_check.cpp'), '-o', exe])
    return exe


def run(exe):
    """case -> (return code, plan, doubles of the image, error text)"""
    out = subprocess.check_output([exe], text=True)
    index = {}
    for line in out.splitlines():
        name, rc, plan, count, error = line.split('\t')
        assert name not in index
        index[name] = (int(rc), plan, int(count), error)
    return index


@pytest.fixture(scope='module')
def checked(tmp_path_factory):
    return run(build(tmp_path_factory.mktemp('gps_terms'), 'gps_terms_check',
                     ['-O2']))


def sequences():
    return [c for k in (2, 3) for c in itertools.product(range(4), repeat=k)]


def read_side(codes):
    """What the kernel is told: slot I is the I-th term in a stable sort by
    kernel code, with the column of its a in a row that holds the terms in
    the caller's order, then s; the column of a sho's q is two after that of
    its a, and 0 (not read) for the other kernels."""
    first = [sum(COLUMNS[c] for c in codes[:i]) for i in range(len(codes))]
    order = sorted(range(len(codes)), key=lambda i: codes[i])
    width = sum(COLUMNS[c] for c in codes) + 1
    numbers = [len(codes)] + [codes[i] for i in order] + \
        [first[i] for i in order] + \
        [first[i] + 2 if codes[i] == 3 else 0 for i in order] + \
        [width - 1, width, sum(STATES[c] for c in codes)]
    return ' '.join(map(str, numbers))


def read_side_one(code):
    """One term's row is (a, l, s[, q]): a in column 0, s in column 2 and a
    sho's q in column 3."""
    from nautilus_amd import device
    names = {v: k for k, v in device.GPS_KERNELS.items()}
    width = device.gps_width(names[code])
    assert width == (4 if code == 3 else 3)
    numbers = [1, code, 0, 3 if code == 3 else 0, 2, width, STATES[code]]
    return ' '.join(map(str, numbers))


def test_cases(checked):
    names = {'k' + ''.join(map(str, c)) for c in sequences()}
    assert len(names) == 16 + 64
    ones = {'one%d' % c for c in range(4)}
    assert set(checked) == names | ones | set(REFUSALS)


def test_every_slot_sits_where_the_kernel_reads_it(checked):
    accepted = set()
    for codes in sequences():
        name = 'k' + ''.join(map(str, codes))
        states = sum(STATES[c] for c in codes)
        if states > 6:
            assert checked[name] == (ERR_ARG, '', 0, TOO_MANY % states), name
            continue
        # the image is pack_gps's own: 4 doubles per datum
        assert checked[name] == (0, read_side(codes), 20, ''), name
        accepted.add(tuple(sorted(codes)))
    assert len(accepted) == 23
    assert len([c for c in accepted if len(c) == 2]) == 10
    # written out: sho, exp, sho is slots exp (column 3), sho (0), sho (5),
    # with the q of the two sho in columns 2 and 7
    assert checked['k303'][1] == '3 0 3 3 3 0 5 0 2 7 8 9 5'
    assert checked['k21'][1] == '2 1 2 2 0 0 0 4 5 5'


def test_one_term_sits_where_the_kernel_reads_it(checked):
    """``plan_gps_one``: the plan of ``nb_gps_create`` for each of the four
    kernels, with the width of ``device.gps_width``."""
    from nautilus_amd import device
    for code in range(4):
        assert checked['one%d' % code] == (0, read_side_one(code), 20, ''), \
            code
    assert sorted(device.GPS_KERNELS.values()) == [0, 1, 2, 3]
    # written out: (a, l, s) and, for sho, (a, l, s, q)
    assert checked['one0'][1] == '1 0 0 0 2 3 1'
    assert checked['one1'][1] == '1 1 0 0 2 3 2'
    assert checked['one2'][1] == '1 2 0 0 2 3 3'
    assert checked['one3'][1] == '1 3 0 3 2 4 2'


def test_refusals(checked):
    for name, message in REFUSALS.items():
        assert checked[name] == (ERR_ARG, '', 0, message), name
        assert 'Gaussian-process series likelihood' in message
    assert len({NULL, COUNT, CODE, TOO_MANY}) == 4


def test_under_the_sanitizers(checked, tmp_path):
    """The same program, built with -fsanitize=address,undefined and run on
    its own: it gives the same lines, and neither sanitizer reports
    anything."""
    exe = build(tmp_path, 'gps_terms_check_san',
                ['-O1', '-g', '-fsanitize=address,undefined',
                 '-fno-sanitize-recover=all', '-fno-omit-frame-pointer'])
    assert run(exe) == checked
