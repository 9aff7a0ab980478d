"""The emulator scores of nb_eval_fast.hip by value, on every entry point,
place and route: ``DeviceBound.neural_score_rows`` (any neural bound, through
an index list or without, with the periodic shift or without) against a long
double evaluation of the same networks (score_cases.py), a row's score against
the same row in any other lane, wavefront, pass, workgroup or list slot, and
the decisions of the staged route's BATCH launch against the scores themselves
-- with the threshold at the median of a cloud and with the threshold ON a
row's score.

The unit of the value tests is the fp64 oracle's own error against the long
double reference on the same rows, ``e_ref`` (test_score_cases.py: one or two
ulp of the score, below 2^-50): the device may be ``K`` times as far off, in
r^2 (relative) and in the score (absolute) separately.

K = 8: the next power of two at or above twice the largest ratio e_dev /
e_ref of one MI355X run over all 51 cases and their neural bounds -- 2.21, in
the score of width(50, 4), m = 0; 2.04 in r^2 (width(128, 1), m = 2); the
median ratio is about 1 (profiles/score_parity/ratios.txt, written by
profiles/tools/score_parity.py).  The device sums in another order and
multiplies by a rounded 1 / scale
where the oracle divides, a few ulp and no orders of magnitude."""

import functools

import numpy as np
import pytest

import accept_cases as ac
import score_cases as sc
from helpers import upload
from test_accept_routes_gpu import _accept, _bound

pytestmark = pytest.mark.gpu

K = 8.0

CASES = ([('per_dim', (d,)) for d in ac.DIMS] +
         [('width', de) for de in sc.WIDTH])


def _ids(case):
    return '%s-%s' % (case[0], '-'.join(str(a) for a in case[1]))


@pytest.fixture(autouse=True)
def gpu_only():
    import torch
    if not torch.cuda.is_available():
        pytest.skip('no GPU')


def _dev(x):
    import torch
    return torch.from_numpy(np.array(x)).cuda()    # (a copy: x is read-only)


@functools.lru_cache(maxsize=None)
def _uploaded(kind, *args):
    if kind == 'per_dim':
        return _bound(args[0], 3, 2)
    return upload(getattr(sc, kind)(*args).ob)


def _host(pair):
    return tuple(t.cpu().numpy() for t in pair)


def ratios(kind, *args):
    """Per neural bound of the case: (e_dev, e_ref), each (r2 relative, score
    absolute) against ``ld_scores`` -- the device through
    ``neural_score_rows`` without an index list, in the frame the sampler
    sees."""
    case, b = getattr(sc, kind)(*args), _uploaded(kind, *args)
    assert b.n_neural == len(case.neural) and b.n_networks == case.E
    xd, out = _dev(case.x), []
    for m, (ref, e_ref) in enumerate(sc.reference(kind, *args)):
        got = _host(b.neural_score_rows(xd, None, m,
                                        recentre=case.shift is not None))
        out.append((sc.errors(*got, ref), e_ref))
    return out


def _within(e_dev, e_ref, what):
    for name, dev, ref in zip(('r2', 'score'), e_dev, e_ref):
        print('%s %s: device %.3g, oracle %.3g, ratio %.2f' % (
            what, name, dev, ref, dev / ref))
        assert dev <= K * ref, (what, name, dev, ref)


@pytest.mark.parametrize('case', CASES, ids=_ids)
def test_scores_against_the_long_double_reference(case):
    """Every neural bound of the case -- the blob offset of m = 1, 2 -- on
    rows inside, outside and far outside its ellipsoid and outside the unit
    cube; and ``neural_score`` is the same launch as m = 0 without a list."""
    import torch
    kind, args = case
    for m, (e_dev, e_ref) in enumerate(ratios(kind, *args)):
        _within(e_dev, e_ref, '%s m=%d' % (_ids(case), m))
    b, xd = _uploaded(kind, *args), _dev(getattr(sc, kind)(*args).x)
    a, c = b.neural_score(xd), b.neural_score_rows(xd, None, 0)
    assert torch.equal(a[0], c[0]) and torch.equal(a[1], c[1])


@pytest.mark.parametrize('d', ac.DIMS)
def test_rows_bit_for_bit(d):
    """A row's (r2, score) does not depend on its lane, wavefront, pass,
    workgroup or slot in an index list: every list of score_cases.py against
    the launch without a list, indexed."""
    import torch
    case, b = sc.per_dim(d), _uploaded('per_dim', d)
    xd = _dev(case.x)
    lists = dict(sc.index_lists())
    if d in sc.LONG_DIMS:
        lists['long'] = sc.long_list()
    source, wide = sc.wide_list()
    x_wide = xd[_dev(source)].contiguous()
    for m in range(2):
        base = b.neural_score_rows(xd, None, m)
        assert all(bool(torch.isfinite(t).all()) for t in base)
        for name, idx in lists.items():
            idx_d = _dev(idx)
            got = b.neural_score_rows(xd, idx_d, m)
            for g, want in zip(got, base):
                assert g.shape == (len(idx),), (name, m)
                assert torch.equal(g, want[idx_d]), (name, m)
            if name == 'one_row':
                for g in got:
                    assert torch.equal(g, g[:1].expand_as(g)), m
        # a list into a longer x, its first and last row included
        got = b.neural_score_rows(x_wide, _dev(wide), m)
        rows = _dev(source[wide])
        for g, want in zip(got, base):
            assert torch.equal(g, want[rows]), ('wide', m)


def test_recentre():
    """The periodic shift inside the kernel: rows in the sampler's frame with
    ``recentre`` and rows the oracle shifted without it, against the long
    double scores of the shifted rows; without a shift in the bound the
    switch changes nothing."""
    import torch
    for d in sc.PERIODIC:
        case, b = sc.periodic(d), _uploaded('periodic', d)
        (ref, e_ref), = sc.reference('periodic', d)
        (e_dev, e_ref2), = ratios('periodic', d)
        assert e_ref2 == e_ref
        _within(e_dev, e_ref, 'periodic d=%d, recentred' % d)
        shifted = _dev(case.shift.transform(case.x))
        got = _host(b.neural_score_rows(shifted, None, 0, recentre=False))
        _within(sc.errors(*got, ref), e_ref,
                'periodic d=%d, shifted by the oracle' % d)
        # (and the unshifted rows are other rows: the shift is not a no-op)
        raw = _host(b.neural_score_rows(_dev(case.x), None, 0))
        assert not np.array_equal(raw[0], got[0])
    for d in (5, 128):
        b, xd = _uploaded('per_dim', d), _dev(sc.per_dim(d).x)
        for m in range(2):
            on = b.neural_score_rows(xd, None, m, recentre=True)
            off = b.neural_score_rows(xd, None, m, recentre=False)
            assert torch.equal(on[0], off[0]) and torch.equal(on[1], off[1])


def _device_values(b, xd):
    return [_host(b.neural_score_rows(xd, None, m))
            for m in range(b.n_neural)]


def _follows_the_scores(b, flags, values):
    """bit 1 = bit 0 & any_m(r2_m < 1 & score_m > threshold_m) on the device's
    own values, for every row; where r2_m lies within 1e-12 of 1 (at most two
    rows, test_accept_routes.py) either side of that rim is taken."""
    bit0, bit1 = (flags & 1) != 0, (flags & 2) != 0
    lo = np.zeros(len(flags), dtype=bool)
    hi = np.zeros(len(flags), dtype=bool)
    for (r2, score), thr in zip(values, b.thresholds):
        edge = np.abs(r2 - 1.0) < ac.R2_TOL
        lo |= (r2 < 1) & ~edge & (score > thr)
        hi |= ((r2 < 1) | edge) & (score > thr)
    open_rows = lo != hi
    assert open_rows.sum() <= 2
    assert flags.max() <= 3
    bad = np.flatnonzero((bit1 != (bit0 & lo)) & ~open_rows)
    assert len(bad) == 0, (bad[:10], [
        (float(s[bad[0]]) - t) for (_, s), t in zip(values, b.thresholds)])
    assert not np.any(bit1 & ~(bit0 & hi))


@pytest.mark.parametrize('d', ac.DIMS)
def test_staged_decisions_follow_the_scores(d):
    """The BATCH launch behind the staged route shows decisions only: they
    are the plain launch's scores against the uploaded thresholds, row for
    row, with no exemption near a threshold."""
    p, b = ac.proposals(d, 3, 2), _bound(d, 3, 2)
    xd = _dev(p.x)
    flags = _accept(b, 'staged', ac.seed_of(d), ac.OFFSET, xd)
    assert np.array_equal(flags & 1, p.keep.astype(np.uint8))
    _follows_the_scores(b, flags, _device_values(b, xd))


N_COPIES = 40


@pytest.mark.parametrize('d', sc.tile_edge_dims())
def test_threshold_sits_on_a_score(d):
    """The threshold of neural bound m put ON the device's score of a row
    whose acceptance emulator m decides alone: score > threshold is false,
    the row is rejected; one step below it is accepted.  40 copies of the row
    behind the proposals (other wavefronts, the ragged last pass of the
    candidate list) decide as the row does."""
    import torch
    case, p, b = ac.build(d, 3, 2), ac.proposals(d, 3, 2), _bound(d, 3, 2)
    seed, n = ac.seed_of(d), ac.N_ROWS
    xd = _dev(p.x)
    flags = _accept(b, 'staged', seed, ac.OFFSET, xd)
    values = _device_values(b, xd)
    r2, score = [v[0] for v in values], [v[1] for v in values]
    for m in range(2):
        piv = np.flatnonzero(sc.pivot_mask((flags & 1) != 0, r2, score,
                                           b.thresholds, m))
        assert len(piv) >= 1, m
        j = int(piv[np.argmin(np.abs(score[m][piv] -
                                     np.median(score[m][piv])))])
        s_j = float(score[m][j])
        x_ext = torch.cat([xd, xd[j:j + 1].expand(N_COPIES, d)]).contiguous()
        for target, want in ((s_j, 0), (float(np.nextafter(s_j, -np.inf)), 1)):
            b2 = upload(sc.with_threshold(case.ob, m, target))
            assert b2.thresholds[m] == target
            assert b2.thresholds[1 - m] == b.thresholds[1 - m]
            f2 = _accept(b2, 'staged', seed, ac.OFFSET, x_ext)
            v2 = _device_values(b2, x_ext)
            for old, new in zip(values, v2):
                assert np.array_equal(old[0], new[0][:n]), (m, want)
                assert np.array_equal(old[1], new[1][:n]), (m, want)
                assert np.all(new[0][n:] == new[0][j])
                assert np.all(new[1][n:] == new[1][j])
            _follows_the_scores(b2, f2, v2)
            assert np.array_equal(f2[:n] & 1, flags & 1)
            assert f2[j] == 1 + 2 * want, (m, want, f2[j])
            copies = f2[n:]
            kept = (copies & 1) != 0
            assert kept.sum() >= 1
            assert np.all(copies[kept] == 1 + 2 * want), (m, want, copies)


def test_argument_errors():
    import torch
    b, xd = _uploaded('per_dim', 5), _dev(sc.per_dim(5).x)
    for m in (-1, b.n_neural):
        with pytest.raises(RuntimeError,
                           match=r'neural bound %d of 2 \(E = 2\)' % m):
            b.neural_score_rows(xd, None, m)
    bare = upload(ac.list_case(5).obs[4])
    assert bare.n_neural == 1 and bare.n_networks == 0
    with pytest.raises(RuntimeError,
                       match=r'neural bound 0 of 1 \(E = 0\)'):
        bare.neural_score_rows(xd, None, 0)
    for idx in ([-1], [0, sc.N_ROWS], [5, 2**40]):
        with pytest.raises(ValueError, match='outside the %d rows' %
                           sc.N_ROWS):
            b.neural_score_rows(xd, idx, 0)
    for idx in ([], torch.zeros(0, dtype=torch.int64, device='cuda')):
        r2, score = b.neural_score_rows(xd, idx, 1)
        assert r2.shape == score.shape == (0,)
        assert r2.dtype == score.dtype == torch.float64 and r2.is_cuda
    # a list of Python ints, numpy ints of another width: one int64 tensor
    r2, score = b.neural_score_rows(xd, np.array([3, 3, 0], dtype=np.int32), 1)
    base = b.neural_score_rows(xd, None, 1)
    assert torch.equal(r2, base[0][[3, 3, 0]])
    assert torch.equal(score, base[1][[3, 3, 0]])
