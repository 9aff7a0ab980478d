"""Membership decisions of every kernel that evaluates |B_inv (x - c)|^2 < 1,
on rows placed on the ellipsoid's rim (rim_cases.py): at distances from
r^2 = 1 that start at twice the derived bound on an fp64 kernel's own
rounding, where a correct kernel cannot flip and one that rounds its matrix,
its centre or its sum to single precision flips every second row.  Every
comparison is exact and on ALL rows: test_rim_cases.py shows on the CPU that
no case has a row within the bound of the rim.

 * value: r^2 of nb_geom.hip and nb_eval_fast.hip through ``neural_score``
   against the long double reference, within the bound row by row;
 * stream: the variants of nb_stream.hip through ``contains_stream``;
 * count and lists: nb_geom.hip's count mode (``member_count``) and the
   geometric stage of nb_cand.hip (``contains``, ``contains_any``,
   ``first_containing``);
 * acceptance: ``accept`` on the fused and on the staged route, pinned and
   read back from ``device.DISPATCHES``;
 * shifted: ``contains`` and ``neural_score_rows(recentre=True)`` behind a
   periodic shift.

Largest used fraction of the bound in the value and shifted tests, one MI355X
run (profiles/rim_parity/ratios.txt): 0.33 at n_dim 1, 0.05 at 16, 0.0044 at
128; the largest error is 2 to 4e-16 throughout."""

import numpy as np
import pytest

import rim_cases as rc
from helpers import upload
from test_accept_routes_gpu import _accept, _counted

pytestmark = pytest.mark.gpu

SEED, OFFSET = 5, 10**10 + 7


@pytest.fixture(autouse=True)
def gpu_only():
    import torch
    if not torch.cuda.is_available():
        pytest.skip('no GPU')


def _dev(x):
    import torch
    return torch.from_numpy(np.array(x)).cuda()    # (a copy: x is read-only)


def _host(t):
    return t.cpu().numpy()


def _same(got, want, what):
    got = np.asarray(got)
    want = np.asarray(want).astype(got.dtype)
    assert got.shape == want.shape, what
    assert np.array_equal(got, want), (what, np.flatnonzero(got != want)[:8])


def _within(case, j, r2, what):
    """|r2 - r2_ref| <= bound on every row, and r2 < 1 as the reference
    decides; returns the largest used fraction of the bound."""
    assert not np.any(case.undecided[j])
    err = np.abs(r2.astype(rc.L) - case.r2[j]).astype(np.float64)
    used = float(np.max(err / case.bound[j]))
    print('%s: largest |r2 - r2_ref| / bound %.4f (largest error %.3g)' % (
        what, used, float(np.max(err))))
    assert np.all(err <= case.bound[j]), (what, used)
    _same(r2 < 1, case.inside[j], what)
    return used


@pytest.mark.parametrize('d', rc.VALUE_DIMS)
def test_r2_value(d):
    """A bound without networks runs nb_geom.hip, one with a dummy network
    nb_eval_fast.hip: both within the bound of the reference on every row."""
    from nautilus_amd import device
    from oracle import mlp_oracle as mo
    case = rc.ellipsoid(d)
    e = case.rims[0]
    ell = device.member(e.c, e.B, e.B_inv)
    plain = device.DeviceBound(d, [], None, False, [dict(ellipsoid=ell)])
    with_net = device.DeviceBound(d, [], None, False, [dict(
        ellipsoid=ell, score_predict_min=0.0,
        mlp=dict(mean=np.zeros(d), scale=np.ones(d),
                 nets=[mo.glorot_init(d, 0)[:2]]))])
    assert plain.n_networks == 0 and with_net.n_networks == 1
    xd = _dev(case.x)
    for name, b in (('nb_geom', plain), ('nb_eval_fast', with_net)):
        r2 = _host(b.neural_score(xd)[0])
        _within(case, 0, r2, 'n_dim %3d %s' % (d, name))


@pytest.mark.parametrize('d', rc.STREAM_DIMS)
def test_stream(d):
    """``contains_stream`` (rim_cases.stream_variant(d) says which kernel):
    the full launch and prefixes that end inside a tile, a unit and a group."""
    case = rc.ellipsoid(d)
    b, xd = upload(case.ob), _dev(case.x)
    full = _host(b.contains_stream(xd))
    _same(full, case.inside[0], rc.stream_variant(d))
    for k in rc.PREFIXES:
        _same(_host(b.contains_stream(xd[:k])), full[:k], k)


@pytest.mark.parametrize('d', rc.ACCEPT_DIMS)
def test_count_and_lists(d):
    """The overlap count with the rim ellipsoid first and second among the
    members and as a mixture's ellipsoid over a subset of the features;
    ``contains`` of the same bounds; exclusion and association with the rim
    bound behind and in front of a far one."""
    import torch
    from nautilus_amd import device
    cases = [rc.union(d, 0), rc.union(d, 1)] + (
        [rc.mixture(d)] if d >= 3 else [])
    for case in cases:
        b, xd = upload(case.ob), _dev(case.x)
        count = b.member_count(xd)
        assert count.dtype == torch.uint8
        _same(_host(count), case.inside[0], case.name)
        _same(_host(b.contains(xd)), case.inside[0], case.name)
    case = rc.ellipsoid(d)
    xd, inside = _dev(case.x), case.inside[0]
    far, rim = upload(rc.far_ellipsoid(d)), upload(case.ob)
    for at, bounds in ((1, [far, rim]), (0, [rim, far])):
        lst = device.DeviceBoundList(bounds)
        _same(_host(lst.contains_any(xd)), inside, at)
        _same(_host(lst.first_containing(xd)), np.where(inside, at, -1), at)


@pytest.mark.parametrize('d', rc.ACCEPT_DIMS)
def test_accept(d):
    """Bit 0 on every row, bit 1 the reference's r^2 decision (the emulator
    accepts every row), the fused and the staged route bit for bit, and the
    emulator asked about exactly the rows inside -- no slack; two neural
    bounds on the staged route; ``contains`` of the same bounds (the
    bounding-sphere screen of the list kernels with the rows on the longest
    semi-axis inside its margin)."""
    case = rc.neural(d, 1)
    b, xd = upload(case.ob), _dev(case.x)
    assert (b.n_neural, b.n_members, b.n_networks) == (1, 1, case.E)
    want = 1 + 2 * case.inside[0].astype(np.uint8)
    flags = {}
    for route in ('fused', 'staged'):
        flags[route], evals = _counted(b, route, SEED, OFFSET, xd)
        _same(flags[route], want, (d, route))
        assert evals == case.E * int(case.inside[0].sum()), (d, route)
    assert np.array_equal(flags['fused'], flags['staged'])
    _same(_host(b.contains(xd)), case.inside[0], d)

    case = rc.neural(d, 2)
    b, xd = upload(case.ob), _dev(case.x)
    assert (b.n_neural, b.n_members, b.n_networks) == (2, 1, case.E)
    either = case.inside[0] | case.inside[1]
    got, evals = _counted(b, 'staged', SEED, OFFSET, xd)
    _same(got, 1 + 2 * either.astype(np.uint8), d)
    assert evals == case.E * int(case.inside[0].sum() + case.inside[1].sum())
    _same(_host(b.contains(xd)), either, d)


@pytest.mark.parametrize('d', rc.SHIFT_DIMS)
def test_shifted(d):
    """Rows in the sampler's frame, the periodic shift inside the kernels:
    ``contains`` and the value of r^2 against the reference of the rows the
    oracle shifted."""
    case = rc.shifted(d)
    b, xd = upload(case.ob), _dev(case.x)
    _same(_host(b.contains(xd)), case.inside[0], d)
    r2 = _host(b.neural_score_rows(xd, None, 0, recentre=True)[0])
    _within(case, 0, r2, 'n_dim %3d shifted' % d)
