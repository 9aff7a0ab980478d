"""Both routes of ``DeviceBound.accept`` and the list evaluation at every
instantiation of nb_eval_fast.hip and nb_cand.hip, with the route PINNED
(``dense_need``) and read back from ``device.DISPATCHES``: the fused kernel
(cube test, ellipsoid and emulators of one neural bound in one pass) and the
staged route (nb_cand.hip + one BATCH launch of nb_eval_fast.hip) against the
oracle's decisions on the same rows (accept_cases.py; union.py:313-319,
nautilus.py:162-169, 212-216, neural.py:115-126) and against each other.

Tolerances are the suite's: proposals to 1e-12, decisions exact outside the
rows whose r^2 lies within 1e-12 of 1 or whose score lies within 1e-9 of the
threshold; test_accept_routes.py shows on the CPU that at most two of the
6000 rows of a case are such rows and that every decision goes both ways."""

import functools
import os

import numpy as np
import pytest

import accept_cases as ac
from helpers import upload

pytestmark = pytest.mark.gpu

ROUTES = ('fused', 'staged')


@pytest.fixture(autouse=True)
def gpu_only():
    import torch
    if not torch.cuda.is_available():
        pytest.skip('no GPU')


@functools.lru_cache(maxsize=None)
def _bound(d, k, m):
    return upload(ac.build(d, k, m).ob)


def _dev(x):
    import torch
    return torch.from_numpy(np.array(x)).cuda()    # (a copy: x is read-only)


def _accept(b, route, seed, offset, xd):
    """Flags of ``xd`` on the route asked for -- and only its kernels ran."""
    from nautilus_amd import device
    if b.n_neural == 1 and b.n_members <= 1:
        b.dense_need = 1.0 if route == 'fused' else 0.0
    else:
        assert route == 'staged'
    before = dict(device.DISPATCHES)
    flags = b.accept(seed, offset, xd).cpu().numpy()
    ran = {key: device.DISPATCHES[key] - before[key] for key in before}
    assert ran == dict(nb_eval_fast_kernel=1,
                       nb_cand_kernel=0 if route == 'fused' else 1), route
    return flags


def _counted(b, route, seed, offset, xd):
    """(flags, emulator point evaluations) of one launch."""
    from nautilus_amd import device
    with device.EvalCounters() as counters:
        flags = _accept(b, route, seed, offset, xd)
    return flags, counters.read()['emulator_point_evals']


def _check_evals(case, p, evals):
    """E x (row, neural bound) pairs whose emulator the oracle asks, give or
    take the rows on the rim of an ellipsoid."""
    want = case.E * sum(int(r.sum()) for r in p.reach)
    slack = case.E * sum(int(e.sum()) for e in p.edge_r2)
    assert abs(evals - want) <= slack, (evals, want, slack)


@pytest.mark.parametrize('d', ac.DIMS)
def test_both_routes_against_the_oracle(d):
    """One outer member, one neural bound: the fused kernel and the staged
    route on the same proposals, for launches below one pass, around it and
    of many passes.  Bit 0 is the cube test, bit 1 the oracle's acceptance,
    the two routes agree bit for bit (nb_cand.hip: same arithmetic in the same
    order), and each asks the emulator about exactly the rows the oracle
    sends there."""
    case, p, b = ac.build(d, 1, 1), ac.proposals(d, 1, 1), _bound(d, 1, 1)
    assert (b.n_neural, b.n_members, b.n_networks) == (1, 1, case.E)
    seed = ac.seed_of(d)
    got = b.propose(seed, ac.OFFSET, ac.N_ROWS).cpu().numpy()
    assert np.allclose(got, p.x, rtol=0, atol=1e-12)
    xd = _dev(p.x)
    for n in (1, 127, 128, 129, ac.N_ROWS):
        flags = {}
        for route in ROUTES:
            part = xd[:n].contiguous()
            if n == ac.N_ROWS:
                flags[route], evals = _counted(b, route, seed, ac.OFFSET,
                                               part)
                _check_evals(case, p, evals)
            else:
                flags[route] = _accept(b, route, seed, ac.OFFSET, part)
            f, keep = flags[route], ~p.edge[:n]
            assert f.shape == (n,) and f.max() <= 3, (route, n)
            assert np.array_equal(f & 1, p.in_cube[:n].astype(np.uint8)), (
                route, n)
            assert np.array_equal((f >> 1)[keep],
                                  p.accept[:n].astype(np.uint8)[keep]), (
                route, n)
        assert np.array_equal(flags['fused'], flags['staged']), n


def _orders(reach):
    """The rows sorted by whether they reach the emulator: all that do first,
    and the two kinds in alternating stripes of one wavefront's tile (16) and
    of one pass (128)."""
    yes, no = np.flatnonzero(reach), np.flatnonzero(~reach)
    out = dict(halves=np.concatenate([yes, no]))
    for w in (16, 128):
        parts = []
        for i in range(0, max(len(yes), len(no)), w):
            parts += [yes[i:i + w], no[i:i + w]]
        out['stripes of %d' % w] = np.concatenate(parts)
    return out


@pytest.mark.parametrize('d', ac.DIMS)
def test_fused_skips_whole_wavefronts_and_passes(d):
    """What a funnel's proposals look like to the fused kernel: wavefronts
    and whole passes none of whose rows reaches the emulator.  Such a
    wavefront skips the network stages but takes part in every barrier and
    in the weight DMA of each of them.  With at most one outer member the
    flags do not depend on the stream position, so the rows may come in any
    order: the flags are the permuted flags of the unordered launch, on both
    routes, and the emulator is asked about as many rows."""
    case, p, b = ac.build(d, 1, 1), ac.proposals(d, 1, 1), _bound(d, 1, 1)
    seed, reach = ac.seed_of(d), p.reach[0]
    assert min(reach.sum(), (~reach).sum()) >= 256      # whole passes of each
    xd = _dev(p.x)
    for route in ROUTES:
        base, evals = _counted(b, route, seed, ac.OFFSET, xd)
        _check_evals(case, p, evals)
        for name, perm in _orders(reach).items():
            assert np.array_equal(np.sort(perm), np.arange(ac.N_ROWS))
            got, evals_p = _counted(b, route, seed, ac.OFFSET,
                                    xd[_dev(perm)].contiguous())
            assert np.array_equal(got, base[perm]), (route, name)
            assert evals_p == evals, (route, name)


@pytest.mark.parametrize('d', ac.DIMS)
def test_cube_edge_on_every_feature(d):
    """Every feature in turn just below 0, at 0, just below 1 and at 1, the
    others at the centre of the neural ellipsoid: the cube test (its map from
    register slot to feature, f = 8 (ks >> 1) + 2 lg + (ks & 1), and the
    padding predicate f < n_dim of the last tile) says out, in, in, out, and
    nothing outside the cube is accepted."""
    case, b = ac.build(d, 1, 1), _bound(d, 1, 1)
    centre = case.neural[0].outer_bound.c
    assert np.all((centre > 0) & (centre < 1))
    x = np.repeat(centre[None, :], 4 * d, axis=0)
    values = [-2.0**-60, 0.0, np.nextafter(1.0, 0.0), 1.0]
    for j in range(d):
        x[4 * j:4 * j + 4, j] = values
    want = np.tile(np.array([0, 1, 1, 0], dtype=np.uint8), d)
    assert np.array_equal(
        np.all((x >= 0) & (x < 1), axis=1).astype(np.uint8), want)
    for route in ROUTES:
        flags = _accept(b, route, ac.seed_of(d), ac.OFFSET, _dev(x))
        assert np.array_equal(flags & 1, want), (
            route, np.flatnonzero((flags & 1) != want))
        assert not np.any((flags >> 1) & ~(flags & 1)), route


SLICES = ((1203, 1904), (5, 38))       # 701 rows from an odd offset, 33 rows


@pytest.mark.parametrize('d', ac.DIMS)
def test_staged_route_with_overlapping_members(d):
    """Three overlapping outer members and two neural bounds: the overlap
    count and the draw u > 1 - 1 / k of the candidate kernel (rows that no
    member contains are kept), two candidate lists, ``contains`` of the same
    bound -- and the same rows in smaller launches (other points per
    wavefront, other list layout) get the same flags."""
    case, p, b = ac.build(d, 3, 2), ac.proposals(d, 3, 2), _bound(d, 3, 2)
    assert (b.n_neural, b.n_members, b.n_networks) == (2, 3, case.E)
    seed = ac.seed_of(d)
    got = b.propose(seed, ac.OFFSET, ac.N_ROWS).cpu().numpy()
    assert np.allclose(got, p.x, rtol=0, atol=1e-12)
    xd = _dev(p.x)
    full, evals = _counted(b, 'staged', seed, ac.OFFSET, xd)
    _check_evals(case, p, evals)
    assert np.array_equal(full & 1, p.keep.astype(np.uint8))
    assert np.array_equal((full >> 1)[~p.edge],
                          p.accept.astype(np.uint8)[~p.edge])
    inside = b.contains(xd).cpu().numpy()
    calm = ~(p.edge | p.edge_outer)
    assert np.array_equal(inside[calm], p.contains[calm])
    for lo, hi in SLICES:
        part = xd[lo:hi].contiguous()
        assert np.array_equal(
            _accept(b, 'staged', seed, ac.OFFSET + lo, part), full[lo:hi])
        assert np.array_equal(b.contains(part).cpu().numpy(), inside[lo:hi])


@pytest.mark.parametrize('d', ac.DIMS)
def test_list_routes(d):
    """Exclusion (any bound) and association (first bound) of a list of ten
    bounds -- periodic shift, no neural bound, no emulator, box limits, no
    member, the unit cube last -- against the oracle's ``contains`` of every
    bound: all rows, 701 rows from an odd offset (block rows over the bounds,
    the byte-wise OR from an unaligned slab) and 33 rows; at once, in slabs
    and in group slices.  And a list short enough for one block row to walk
    it."""
    from nautilus_amd import device
    c = ac.list_case(d)
    xd = _dev(c.x)
    devs = [upload(ob) for ob in c.obs]

    def check(lst, inside, slices):
        want_any = inside.any(axis=0)
        want_first = np.where(want_any, np.argmax(inside, axis=0), -1)
        for lo, hi in slices:
            part, keep = xd[lo:hi].contiguous(), ~c.edge[lo:hi]
            got_any = lst.contains_any(part).cpu().numpy()
            got_first = lst.first_containing(part).cpu().numpy()
            assert np.array_equal(got_any[keep], want_any[lo:hi][keep])
            assert np.array_equal(got_first[keep], want_first[lo:hi][keep])

    lst = device.DeviceBoundList(devs)
    slices = ((0, len(c.x)),) + SLICES
    check(lst, c.inside, slices)
    old = device.WORK_BYTES
    device.WORK_BYTES = 1 << 18
    try:
        check(lst, c.inside, slices)
    finally:
        device.WORK_BYTES = old
    os.environ['NB_LIST_SLICE_GROUPS'] = '5'
    try:
        check(lst, c.inside, slices)
    finally:
        del os.environ['NB_LIST_SLICE_GROUPS']
    # fewer than eight bounds: no block rows over the bounds
    short = [1, 3, 4, 5, 7, 9]
    check(device.DeviceBoundList([devs[i] for i in short]), c.inside[short],
          slices)
