"""The host packers (nautilus_amd/csrc/nb_pack.h, the very header nb_api.hip
includes), built for the host by tests/pack_check.cpp: every image the kernels
read -- bound blobs, prior tables, likelihood tables -- and every refusal.

Two independent checks.  tests/golden/pack.npz holds what the packing code
gave while it still lived in nb_api.hip (recorded by building pack_check.cpp
against that file, with a stand-in for the HIP runtime whose allocations are
host memory): return code, error text and image of every case must be the
recorded ones.  And the layout formulas of nb_layout.h are written out again
here in numpy: every input value has to sit where its kernel reads it, with
zeros in the rest of each tile region."""

import json
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.abspath(os.path.dirname(__file__)))
GOLDEN = os.path.join(ROOT, 'tests', 'golden', 'pack.npz')

TILE, HDR = 256, 32
H = (100, 50, 20, 1)                     # outputs of the four layers
HT = (7, 4, 2, 1)                        # ... in 16-wide tiles


@pytest.fixture(scope='module')
def golden():
    with np.load(GOLDEN) as z:
        index = json.loads(str(z['index']))
        return index, {k: z[k] for k in z.files if k != 'index'}


@pytest.fixture(scope='module')
def packed(tmp_path_factory):
    """(index, images) of the program's run of every case"""
    cxx = next((c for c in ('g++', 'c++', 'clang++', 'hipcc')
                if shutil.which(c)), None)
    assert cxx is not None, 'no C++ compiler (the build needs hipcc anyway)'
    tmp = tmp_path_factory.mktemp('pack')
    exe = str(tmp / 'pack_check')
    subprocess.check_call(
        [cxx, '-x', 'c++', '-std=c++17', '-O2',
         '-I', os.path.join(ROOT, 'nautilus_amd', 'csrc'),
         '-I', os.path.join(ROOT, 'include'),
         os.path.join(ROOT, 'tests', 'pack_check.cpp'), '-o', exe])
    out = subprocess.check_output([exe, 'all', str(tmp)], text=True)
    index, images = {}, {}
    for line in out.splitlines():
        name, rc, level, nbytes, error = line.split('\t')
        assert name not in index
        index[name] = dict(rc=int(rc), level=int(level), error=error)
        img = np.fromfile(str(tmp / (name + '.bin')), dtype=np.uint8)
        assert img.size == int(nbytes)
        if int(rc) == 0:
            images[name] = img
    return index, images


def doubles(img):
    return img[:img.size // 8 * 8].view(np.float64)


# ---- against the recording ---------------------------------------------------

# The doubles that pass through the host's libm, which the project does not
# pin: they may differ from the recording by one ulp.  The member CDF of a
# union with volumes (all but its last entry, which is set to 1), and of the
# prior-table rows 2 .. 6 those libm gives: rows 2, 3 of a column of kind 2
# (logarithms) and rows 4 .. 6 of kinds 5 and 6 (rows 2, 3 are the interval).
def libm_doubles(name, img):
    if name == 'b2':
        return [HDR + 0]                         # K = 2: cdf[0]
    if name.startswith('prior_'):
        kinds = {'prior_8': (0, 1, 2, 3, 4, 5, 5, 5), 'prior_tails': (5, 5, 5),
                 'prior_level0': (0, 2), 'prior_keys': (0, 1)}[name]
        d = len(kinds)
        return [r * d + j for j, k in enumerate(kinds) if k in (2, 5)
                for r in ((2, 3) if k == 2 else (4, 5, 6))]
    return []


def ordered(x):
    """doubles as integers whose order is that of the doubles"""
    i = x.view(np.int64)
    return np.where(i < 0, np.int64(-2 ** 63) - i, i)


def test_cases_are_the_recorded_ones(packed, golden):
    assert sorted(packed[0]) == sorted(golden[0])
    assert sorted(packed[1]) == sorted(golden[1])
    assert len(golden[0]) == 71 and len(golden[1]) == 27


def test_return_codes_and_messages(packed, golden):
    for name, want in golden[0].items():
        assert packed[0][name] == want, name
    refusals = [v['error'] for v in golden[0].values() if v['rc'] != 0]
    assert len(refusals) == 44 and all(refusals)
    # the description with two defects: the periodic index is looked at first
    assert golden[0]['b_two_defects']['error'] == \
        'periodic index 4 out of range'
    assert golden[0]['b_idx_order']['error'].startswith('idx_ell must be')


def test_prior_levels(packed):
    level = {k: v['level'] for k, v in packed[0].items()}
    assert level['prior_level0'] == 0
    assert level['prior_8'] == 1 and level['prior_keys'] == 1
    assert level['prior_tails'] == 2


def test_images_are_the_recorded_ones(packed, golden):
    for name, want in golden[1].items():
        got = packed[1][name]
        assert got.size == want.size, name
        loose = libm_doubles(name, got)
        g, w = doubles(got).copy(), doubles(want).copy()
        if loose:
            assert np.all(np.isfinite(w[loose])), name
            assert np.abs(ordered(g[loose]) - ordered(w[loose])).max() <= 1, \
                (name, g[loose], w[loose])
            g[loose] = w[loose]
        # every other double as bits, and the bytes after the last double
        assert np.array_equal(g.view(np.uint8), w.view(np.uint8)), name
        assert np.array_equal(got[g.size * 8:], want[g.size * 8:]), name


def test_prior_kind6_and_bytes(packed):
    img = packed[1]['prior_tails']
    assert img.size == (8 * 3 + 1) * 8 + 4 + 3
    assert list(img[-3:]) == [6, 6, 6]           # rewritten from kind 5
    par = doubles(img)[:24].reshape(8, 3)
    assert np.array_equal(par[2], [36.0, 36.0, 36.0])     # mirrored interval
    assert np.array_equal(par[3], [40.0, 40.0, np.inf])
    assert np.array_equal(par[7], [1.0, -1.0, 1.0])
    img = packed[1]['prior_keys']
    assert np.array_equal(doubles(img)[16:18], [0.375, 1.375])
    assert list(img[18 * 8:18 * 8 + 8].view(np.int32)) == [-1, 1]
    assert list(img[-2:]) == [0, 1]


# ---- against the layout formulas of nb_layout.h, written out again -----------

def slot(f):
    f = np.asarray(f, dtype=int)
    return 16 * (f // 16) + 4 * (2 * ((f // 8) % 2) + f % 2) + (f % 8) // 2


def ell_values(e, n):
    """B_inv, B, c of ellipsoid e of pack_check.cpp over n dimensions"""
    i, j = np.indices((n, n))
    low = j <= i
    return (np.where(low, 1000.0 * (1 + e) + i + j / 1024.0, 0.0),
            np.where(low, 1000.0 * (11 + e) + i + j / 1024.0, 0.0),
            1000.0 * (21 + e) + np.arange(n) + 0.5)


def tri_tiles(lower, dt):
    """the dt (dt + 1) / 2 tiles of a lower-triangular matrix (stream block,
    mixture record)"""
    n = lower.shape[0]
    out = np.zeros(dt * (dt + 1) // 2 * TILE)
    h, k = np.nonzero(np.tril(np.ones((n, n), bool)))
    ht, kt, kk = h // 16, k // 16, k % 16
    s, lg = 2 * (kk // 8) + kk % 2, (kk % 8) // 2
    at = (ht * (ht + 1) // 2 + kt) * TILE + s * 64 + lg * 16 + h % 16
    assert len(np.unique(at)) == at.size
    out[at] = lower[h, k]
    return out


def ell_block(e, idx, n_dim, dt, boxed, word1):
    """an ell block: ellipsoid e over the dimensions idx"""
    dp, idx = 16 * dt, np.asarray(idx, dtype=int)
    b_inv, _, c = ell_values(e, len(idx))
    lo, hi, cc = np.full(dp, -np.inf), np.full(dp, np.inf), np.zeros(dp)
    box = [f for f in range(n_dim) if boxed and f not in idx]
    lo[slot(box)], hi[slot(box)] = 0.0, 1.0
    cc[slot(idx)] = c
    tiles = np.zeros(dt * dt * TILE)
    i, j = np.nonzero(np.tril(np.ones((len(idx),) * 2, bool)))
    h, k = idx[i], idx[j]
    sl = slot(k)
    ks, lg = sl // 4, sl % 4
    at = ((ks // 4) * dt + h // 16) * TILE + (ks % 4) * 64 + lg * 16 + h % 16
    assert len(np.unique(at)) == at.size
    tiles[at] = b_inv[i, j]
    if word1 is None:
        word1 = np.array([1 if box else 0], np.int64).view(np.float64)[0]
    head = np.array([len(idx)], np.int64).view(np.float64)
    return np.concatenate([head, [word1], lo, hi, cc, tiles])


def net_tiles(m, e, n_dim, kt1):
    """the tiles of network e of neural bound m"""
    out = []
    rows = (n_dim,) + H[:3]
    for l, (kt_n, ht_n) in enumerate(zip((kt1,) + HT[:3], HT)):
        k, h = np.indices((rows[l] + 1, H[l]))           # bias: row k = rows
        value = 100000.0 * (8 * m + 4 * e + l + 1) + 0.25 + 1000.0 * k + h
        at = ((k // 16) * ht_n + h // 16) * TILE + (k % 16) * 16 + h % 16
        tiles = np.zeros(kt_n * ht_n * TILE)
        assert len(np.unique(at)) == at.size and at.max() < tiles.size
        tiles[at] = value
        out.append(tiles)
    return np.concatenate(out)


def i64(x):
    return np.ascontiguousarray(x).view(np.int64)


# the bounds of pack_check.cpp: members (idx_ell, free_dims), neural bounds
# (networks or None, radius given)
BOUNDS = {
    'b1': dict(n_dim=1, members=[(range(1), 0)]),
    'b2': dict(n_dim=16, members=[(range(16), 0), ([0, 3, 7, 8, 15], 0)],
               cube=True, neural=[(2, True)]),
    'b3': dict(n_dim=15, neural=[(1, False)]),
    'b4': dict(n_dim=17, members=[(range(17), 0), ([], 1)],
               neural=[(1, True)], periodic=[0, 16]),
    'b5': dict(n_dim=33, members=[(range(33), 0)]),
    'b6': dict(n_dim=3, members=[(range(3), 0)],
               neural=[(1, True), (1, True)]),
    'b7': dict(n_dim=2, neural=[(None, True)]),
}


@pytest.mark.parametrize('name', sorted(BOUNDS))
def test_bound_blob(packed, name):
    case = BOUNDS[name]
    n_dim = case['n_dim']
    members = [(list(i), f) for i, f in case.get('members', [])]
    neural, cube = case.get('neural', []), case.get('cube', False)
    periodic = case.get('periodic', [])
    blob = doubles(packed[1][name])
    K, M = len(members), len(neural)
    E = (neural[0][0] or 0) if M else 0
    dt, kt1 = (n_dim + 15) // 16, (n_dim + 1 + 15) // 16
    dp = 16 * dt
    ell = 2 + 3 * dp + dt * dt * TILE
    net = (kt1 * 7 + 7 * 4 + 4 * 2 + 2) * TILE
    nstride = ell + 2 + 2 * dp + E * net
    dstride = 2 + 4 * dp + dp * (dp + 1) // 2 + 16
    single = K == 1 and M == 0 and not cube and len(members[0][0]) == n_dim
    off_cdf = HDR
    off_ulo = off_cdf + (max(K, 1) + 1) // 2 * 2
    off_uhi = off_ulo + dp
    off_members = off_uhi + dp
    off_neural = off_members + K * ell
    off_draw = off_neural + M * nstride
    off_stream = off_draw + K * dstride
    off_shift = off_stream + (dp + dt * (dt + 1) // 2 * TILE if single else 0)
    total = off_shift + (2 * dp if periodic else 0)
    assert blob.size == total
    assert list(i64(blob[:20])) == [
        n_dim, dt, K, int(cube), M, E, off_cdf, off_ulo, off_uhi, off_members,
        ell, off_neural, nstride, off_draw, dstride, net, kt1, total,
        off_stream if single else 0, off_shift if periodic else 0]
    assert not blob[20:HDR].any()
    # what the case pins
    assert (dt, kt1) == {'b1': (1, 1), 'b2': (1, 2), 'b3': (1, 1),
                         'b4': (2, 2), 'b5': (3, 3), 'b6': (1, 1),
                         'b7': (1, 1)}[name]

    # member CDF (uniform without volumes: no libm) and the union's cube
    if K and name != 'b2':
        assert np.array_equal(blob[off_cdf:off_cdf + K],
                              np.arange(1, K + 1) / K)
    if name == 'b2':
        p = np.exp(np.array([-1.5, -2.25]) + 1.5)
        assert abs(blob[off_cdf] - p[0] / p.sum()) < 1e-15
        assert blob[off_cdf + 1] == 1.0
    lim = np.full(dp, np.inf)
    if cube:
        lim[slot(np.arange(n_dim))] = 1.0
    assert np.array_equal(blob[off_uhi:off_uhi + dp], lim)
    assert np.array_equal(blob[off_ulo:off_ulo + dp],
                          np.where(np.isinf(lim), -np.inf, 0.0))

    for m, (idx, free) in enumerate(members):
        at = off_members + m * ell
        assert np.array_equal(
            blob[at:at + ell].view(np.int64),
            ell_block(m, idx, n_dim, dt, not free, None).view(np.int64)), m
        # draw block
        at = off_draw + m * dstride
        _, b, c = ell_values(m, len(idx))
        rest = [f for f in range(n_dim) if f not in idx]
        cube_dims = [] if free else rest
        ints = i64(blob[at:at + 2 + 3 * dp])
        assert list(ints[:2]) == [len(idx), len(cube_dims)]
        assert list(ints[2:2 + len(idx)]) == idx
        assert list(ints[2 + dp:2 + dp + len(cube_dims)]) == cube_dims
        column = np.zeros(n_dim, int)
        column[idx] = np.arange(len(idx))
        column[rest] = len(idx) + np.arange(len(rest))
        assert list(ints[2 + 2 * dp:2 + 2 * dp + n_dim]) == list(column)
        assert np.array_equal(blob[at + 2 + 3 * dp:at + 2 + 3 * dp + len(idx)],
                              c)
        i, j = np.nonzero(np.tril(np.ones((len(idx),) * 2, bool)))
        tri = np.zeros(dp * (dp + 1) // 2 + 16)
        tri[i * (i + 1) // 2 + j] = b[i, j]
        assert np.array_equal(blob[at + 2 + 4 * dp:at + dstride], tri)

    for m, (networks, radius) in enumerate(neural):
        at = off_neural + m * nstride
        r2 = 7.5 + m if radius else blob[at + 1]
        assert np.array_equal(
            blob[at:at + ell].view(np.int64),
            ell_block(5 + m, range(n_dim), n_dim, dt, False,
                      r2).view(np.int64))
        if not radius:
            # fallback: at least the largest squared semi-axis of B
            b = ell_values(5 + m, n_dim)[1]
            top = np.linalg.eigvalsh(b @ b.T)[-1]
            assert top <= r2 <= (b * b).sum() * (1 + 2e-9)
        assert blob[at + ell] == (0.625 + m) - 1e-9 and blob[at + ell + 1] == 0
        mean, scale = np.zeros(dp), np.ones(dp)
        if networks is not None:
            f = np.arange(n_dim)
            mean[:n_dim] = 31000.0 + 1000.0 * m + f + 0.25
            scale[:n_dim] = 1.0 / (41000.0 + 1000.0 * m + f + 0.125)
        at += ell + 2
        assert np.array_equal(blob[at:at + dp], mean)
        assert np.array_equal(blob[at + dp:at + 2 * dp], scale)
        for e in range(E):
            w = at + 2 * dp + e * net
            assert np.array_equal(blob[w:w + net], net_tiles(m, e, n_dim, kt1))

    if single:
        b_inv, _, c = ell_values(0, n_dim)
        want = np.concatenate([c, np.zeros(dp - n_dim), tri_tiles(b_inv, dt)])
        assert np.array_equal(blob[off_stream:off_shift], want)
    if periodic:
        shift, on = np.zeros(dp), np.zeros(dp)
        shift[slot(periodic)] = -(0.125 + np.arange(len(periodic)) / 16.0) + 0.5
        on[slot(periodic)] = 1.0
        assert np.array_equal(blob[off_shift:], np.concatenate([shift, on]))


@pytest.mark.parametrize('n_dim, n_comp', [(1, 1), (17, 2), (33, 2)])
def test_mixture_records(packed, n_dim, n_comp):
    img = doubles(packed[1]['mix_%d_%d' % (n_dim, n_comp)])
    dt = (n_dim + 15) // 16
    tail = (16 * dt + 1 + 127) // 128 * 128
    nt = dt * (dt + 1) // 2 * TILE
    assert img.size == n_comp * (nt + tail)
    h, k = np.indices((n_dim, n_dim))
    for c in range(n_comp):
        rec = img[c * (nt + tail):(c + 1) * (nt + tail)]
        li = np.where(k <= h, 1000.0 * (1 + c) + h + k / 1024.0, 0.0)
        want = np.zeros(tail)
        want[:n_dim] = 500.0 + 100.0 * c + np.arange(n_dim) + 0.5
        want[16 * dt] = -0.75 - c
        assert np.array_equal(rec, np.concatenate([tri_tiles(li, dt), want]))


def operand_tiles(matrix, panel, lower):
    """row-streaming operand tiles of a P x K matrix: panels of `panel` row
    tiles; per panel its k-tiles (lower: 0 .. the panel's last row tile);
    per k-tile the panel's row tiles; element (l, c) of a tile at
    (c % 4) * 64 + (c // 4) * 16 + l"""
    p, ks = matrix.shape
    dt, nkt = (p + 15) // 16, (ks + 15) // 16
    padded = np.zeros((16 * dt, 16 * nkt))
    padded[:p, :ks] = matrix
    l, c = np.indices((16, 16))
    at = ((c % 4) * 64 + (c // 4) * 16 + l).ravel()
    assert sorted(at) == list(range(TILE))
    out = []
    for r0 in range(0, dt, panel):
        nrt = min(panel, dt - r0)
        for kt in range(r0 + nrt if lower else nkt):
            for rt in range(r0, r0 + nrt):
                tile = np.zeros(TILE)
                tile[at] = padded[16 * rt:16 * rt + 16,
                                  16 * kt:16 * kt + 16].ravel()
                out.append(tile)
    return np.concatenate(out)


@pytest.mark.parametrize('n', [1, 16, 17, 257])
def test_chi2_table(packed, n):
    img = doubles(packed[1]['chi2_%d' % n])
    dt = (n + 15) // 16
    w_off = (16 * dt + 127) // 128 * 128
    h, k = np.indices((n, n))
    tiles = operand_tiles(np.where(k <= h, 1.0 + 1024.0 * h + k, 0.0), 16, True)
    # 257: a panel of 16 row tiles (16 k-tiles), then one of 1 (17 k-tiles)
    assert tiles.size == {1: 1, 16: 1, 17: 4, 257: 273}[n] * TILE
    head = np.zeros(w_off)
    head[:n] = 3000000.0 + np.arange(n)
    assert np.array_equal(img, np.concatenate([head, tiles]))


def test_small_tables(packed):
    t = lambda name: doubles(packed[1][name])
    three = np.arange(3)
    assert np.array_equal(t('chi2_diag_3'),
                          np.concatenate([3000000.0 + three, 0.5 + three]))
    counts = np.array([2000000.0, 0.0, 2000002.0])
    inverse = np.array([1 / 2000000.0, 0.0, 1 / 2000002.0])
    assert np.array_equal(t('po_3'), np.concatenate(
        [counts, inverse, np.ones(3), np.zeros(3)]))
    assert np.array_equal(t('po_3_tables'), np.concatenate(
        [counts, inverse, 4000000.0 + three, 5000000.0 + three]))
    assert np.array_equal(t('noise_3'),
                          np.concatenate([3000000.0 + three, np.zeros(3)]))
    assert np.array_equal(t('noise_3_sigma2'),
                          np.concatenate([3000000.0 + three, 0.5 + three]))


@pytest.mark.parametrize('n, n_src', [(1, 1), (16, 16), (17, 5), (257, 17)])
def test_fold_table(packed, n, n_src):
    img = doubles(packed[1]['fold_%d_%d' % (n, n_src)])
    dt = (n + 15) // 16
    pp = 16 * dt
    j = np.arange(n)
    table = np.zeros((4, pp))
    table[2] = 1.0
    table[0, :n] = 2000000.0 + j
    table[1, :n] = 1.0 / (2000000.0 + j)
    table[2, :n] = 4000000.0 + j
    table[3, :n] = 5000000.0 + j
    jj, c = np.indices((n, n_src))
    tiles = operand_tiles(1.0 + 1024.0 * jj + c, 16, False)
    assert np.array_equal(img, np.concatenate([table.ravel(), tiles]))
