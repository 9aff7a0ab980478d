"""Which instantiation the launchers pick (nautilus_amd/csrc/nb_dispatch.h, the
very header the kernel files include), built for the host by
tests/dispatch_check.cpp: the tile-count dispatcher inside and outside its
range, and the rule of the last, partly filled tile, against the formulas
written out again here and against the copies the GPU tests lean on
(``device.mixture_launch_shape``, ``rim_cases.stream_variant``,
``accept_cases.instantiation``)."""

import os
import shutil
import subprocess

import pytest

import accept_cases
import rim_cases
from nautilus_amd import device

ROOT = os.path.dirname(os.path.abspath(os.path.dirname(__file__)))
NB_OK, NB_ERR_UNSUPPORTED = 0, 3         # nb_layout.h


@pytest.fixture(scope='module')
def lines(tmp_path_factory):
    cxx = next((c for c in ('g++', 'c++', 'clang++', 'hipcc')
                if shutil.which(c)), None)
    assert cxx is not None, 'no C++ compiler (the build needs hipcc anyway)'
    path = str(tmp_path_factory.mktemp('dispatch') / 'dispatch_check')
    subprocess.check_call(
        [cxx, '-x', 'c++', '-std=c++17', '-O2',
         '-I', os.path.join(ROOT, 'nautilus_amd', 'csrc'),
         os.path.join(ROOT, 'tests', 'dispatch_check.cpp'), '-o', path])
    out = subprocess.check_output([path], text=True)
    return [line.split() for line in out.splitlines()]


def expected_row(n_dim):
    """(DT, KL, SMALL): KL counts the k-steps of 4 that hold a real feature,
    in pairs (half tiles of 8 features); SMALL = 1..4 rows in the last tile"""
    dt = -(-n_dim // 16)
    last = n_dim - 16 * (dt - 1)             # real rows of the last tile, 1..16
    kl = 4 * dt if last > 8 else 4 * dt - 2
    return dt, kl, last <= 4


def test_row_dispatch(lines):
    rows = {int(f[1]): [int(v) for v in f[2:]] for f in lines if f[0] == 'row'}
    assert sorted(rows) == list(range(1, 129))
    seen = set()
    for n_dim, (rc, dt, kl, small, tail_kl, tail_small) in rows.items():
        want = expected_row(n_dim)
        assert rc == NB_OK
        assert (dt, kl, bool(small)) == want, n_dim
        # the values nb_tail_of returns are the tags the dispatcher passes
        assert (tail_kl, bool(tail_small)) == want[1:], n_dim
        assert (dt, kl, bool(small)) == \
            device.mixture_launch_shape(n_dim, 1)[:3], n_dim
        assert (dt, kl, bool(small)) == rim_cases.stream_variant(n_dim)[:3]
        # nb_cand.hip: the same SMALL, but never at one tile
        assert (dt > 1 and bool(tail_small)) == \
            accept_cases.instantiation(n_dim)['cand']['SMALL'], n_dim
        seen.add((dt, kl, bool(small)))
    # exactly the three variants per tile count that are compiled
    assert seen == {(dt, kl, small) for dt in range(1, 9) for kl, small in
                    ((4 * dt, False), (4 * dt - 2, True), (4 * dt - 2, False))}
    over, = [f for f in lines if f[0] == 'over']
    assert [int(v) for v in over[1:]] == [129, NB_ERR_UNSUPPORTED, 1]


@pytest.mark.parametrize('max_tiles', [8, 9])
def test_tile_dispatch(lines, max_tiles):
    got = {int(f[2]): [int(v) for v in f[3:]] for f in lines
           if f[0] == 'tile' and int(f[1]) == max_tiles}
    assert sorted(got) == list(range(-1, 11))
    for tiles, (rc, chosen, error) in got.items():
        if 1 <= tiles <= max_tiles:
            assert (rc, chosen, error) == (NB_OK, tiles, 0), tiles
        else:
            # no kernel runs, least of all the largest one
            assert (rc, chosen, error) == (NB_ERR_UNSUPPORTED, 0, 1), tiles
