"""Bounds, rows and index lists of the emulator-score tests, with a long
double reference of the scores.  Plain numpy and the oracle, no device: shared
by test_score_cases.py (the recipe against its floors, on the CPU) and
test_score_rows_gpu.py (``DeviceBound.neural_score_rows`` and the staged
route's decisions against these values).

``ld_scores`` restates bounds/neural.py:115-120 and neural.py:100-116 in
``np.longdouble`` (64 bits of mantissa on x86): the fp64 parameters and rows
are converted exactly and nothing is rounded to fp64 on the way.  The fp64
oracle agrees with it to an ulp or two of the score; what a device kernel may
deviate is counted in multiples of that error (test_score_rows_gpu.py).

Cases (``Case``: ``name``, ``d``, ``E``, ``ob`` the ONautilus to upload,
``neural`` its ONeural bounds, ``shift`` or None, ``x`` the N_ROWS rows in the
frame the sampler sees):

 * ``per_dim(d)``: ``accept_cases.build(d, 3, 2)``, d in ``accept_cases.DIMS``;
 * ``width(d, E)``: three neural bounds of E networks, ``WIDTH`` -- the blob
   offset of m = 2, the network loop with its last iteration alone (E = 1) and
   at its longest (E = 8), layer 1 in one stage (d < 80) and in two K chunks,
   one (d > 80) and two list tiles per wavefront;
 * ``periodic(d)``: bound 1 of ``accept_cases.list_case(d)``, ``PERIODIC``: a
   phase shift on features 0 and d - 1.

Rows: around every neural ellipsoid in turn at radii sqrt(0.45) to sqrt(1.6)
of it (directions uniform on the sphere, so r^2 is spread evenly over both
sides of the rim whatever n_dim is), N_FAR rows at 2 to 4 radii and N_CUBE
rim rows with one coordinate moved out of the unit cube, permuted; in the
periodic cases N_WRAP rows more whose periodic coordinate lies across the
boundary.  (The hidden activations, and with them the rounding error of any
fp64 evaluation, grow with the radius: at 10 radii the oracle itself is
1e-15 off the long double score, above the 2^-50 asked of it in
test_score_cases.py; at 4 it stays below 7e-16.)  N_ROWS = 293 = two 128-row
passes of nb_eval_fast.hip and a ragged one of 37."""

import copy
import functools
import types

import numpy as np

import accept_cases as ac
from oracle import bounds_oracle as bo

L = np.longdouble

N_ROWS, N_FAR, N_CUBE, N_WRAP = 293, 6, 6, 6
WIDTH = ((5, 1), (50, 4), (80, 8), (100, 8), (128, 1), (128, 4))
PERIODIC = (1, 5, 17, 64, 128)
PREFIXES = (1, 15, 16, 17, 127, 128, 129)
N_LONG, N_WIDE = 32901, 1000
LONG_DIMS = (5, 128)
MIN_PIVOTS = 10


# ---- the reference --------------------------------------------------------

def ld_scores(nb, x, shift=None):
    """(r2, score) of the rows ``x`` under the ONeural ``nb`` in long double.
    ``shift``: an OPhaseShift the oracle applies to the rows first (in fp64,
    as nautilus.py:162-163 does: the shifted row is the input)."""
    if shift is not None:
        x = shift.transform(x)
    ell, em = nb.outer_bound, nb.emulator
    y = (x.astype(L) - ell.c.astype(L)) @ ell.B_inv.astype(L).T
    r2 = np.sum(y * y, axis=1)
    h0 = (y - em.mean.astype(L)) / em.scale.astype(L)
    total = np.zeros(len(x), dtype=L)
    for net in em.networks:
        h, last = h0, len(net.coefs) - 1
        for i, (w, b) in enumerate(zip(net.coefs, net.intercepts)):
            h = h @ np.asarray(w).astype(L) + np.asarray(b).astype(L)
            if i != last:
                h = np.maximum(h, L(0))
        total = total + h[:, 0]
    return r2, total / L(len(em.networks))


def oracle_scores(nb, x, shift=None):
    """The same in the fp64 oracle's own arithmetic (basic.py:340,
    neural.py:100-116)."""
    if shift is not None:
        x = shift.transform(x)
    y = nb.outer_bound.transform(x)
    return np.sum(y**2, axis=1), nb.emulator.predict(y)


def errors(r2, score, ref):
    """(largest relative error of r2, largest absolute error of the score) of
    fp64 values against ``ref = ld_scores(...)``, as Python floats."""
    r2_ref, score_ref = ref
    e_r2 = np.max(np.abs(np.asarray(r2).astype(L) - r2_ref) / r2_ref)
    e_score = np.max(np.abs(np.asarray(score).astype(L) - score_ref))
    return float(e_r2), float(e_score)


# ---- rows -------------------------------------------------------------------

def _rows(neural, rng, d, free):
    """N_ROWS rows in the bounds' frame; ``free``: the features that may
    leave the unit cube."""
    n_rim = N_ROWS - N_FAR
    owner = np.arange(n_rim) % len(neural)
    radius = np.sqrt(rng.uniform(0.45, 1.6, size=N_ROWS))
    radius[n_rim:] = rng.uniform(2.0, 4.0, size=N_FAR)
    owner = np.concatenate([owner, np.arange(N_FAR) % len(neural)])
    u = rng.normal(size=(N_ROWS, d))
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    x = np.empty((N_ROWS, d))
    for j, nb in enumerate(neural):
        sel = owner == j
        x[sel] = nb.outer_bound.transform(radius[sel, None] * u[sel],
                                          inverse=True)
    if len(free) > 0:
        rows = rng.choice(n_rim, size=N_CUBE, replace=False)
        cols = rng.choice(free, size=N_CUBE)
        x[rows, cols] = np.where(np.arange(N_CUBE) % 2 == 0,
                                 -rng.uniform(0.05, 0.4, size=N_CUBE),
                                 1.0 + rng.uniform(0.0, 0.4, size=N_CUBE))
    return x[rng.permutation(N_ROWS)]


def _case(name, d, e, ob, rng):
    shift = ob.shift
    per = np.zeros(d, dtype=bool)
    if shift is not None:
        per[shift.periodic] = True
    x = _rows(ob.neural_bounds, rng, d, np.flatnonzero(~per))
    if shift is not None:             # into the frame the sampler sees
        x[:, per] %= 1.0
        # N_WRAP rows with a periodic coordinate on the far side of the
        # boundary: p + (centre - 0.5) leaves [0, 1) below 0.5 - centre
        # (centre < 0.5) or from 1.5 - centre on
        rows = rng.choice(N_ROWS, size=N_WRAP, replace=False)
        which = rng.integers(0, len(shift.periodic), size=N_WRAP)
        c = shift.centers[which]
        t = rng.uniform(0.05, 0.95, size=N_WRAP)
        x[rows, shift.periodic[which]] = np.where(
            c < 0.5, t * (0.5 - c), 1.0 - t * (c - 0.5))
        x = shift.transform(x, inverse=True)
    x.setflags(write=False)
    return types.SimpleNamespace(name=name, d=d, E=e, ob=ob, shift=shift,
                                 neural=ob.neural_bounds, x=x)


@functools.lru_cache(maxsize=None)
def per_dim(d):
    c = ac.build(d, 3, 2)
    return _case('d%d' % d, d, c.E, c.ob, np.random.default_rng(7000 + d))


@functools.lru_cache(maxsize=None)
def width(d, e):
    """One outer member, three neural bounds of ``e`` Glorot networks each."""
    rng = np.random.default_rng(100 * d + e)
    spread = 0.25 / np.sqrt(d + 2.0)
    neural, members = [], []
    for j in range(3):
        centre = 0.5 + 0.15 * spread * rng.normal(size=d)
        b_mat = np.tril(rng.normal(size=(d, d)) * 0.01) + np.eye(d) * 0.25
        if j == 0:
            members.append(bo.OEllipsoid.from_params(
                centre, (1.0 + 0.7 / d) * b_mat))
        neural.append(ac._neural(rng, centre, b_mat,
                                 [e * j + i for i in range(e)],
                                 1.0 / np.sqrt(d + 2.0), 0.5))
    ob = bo.ONautilus.from_parts(bo.OUnion.from_members(members, unit=True),
                                 neural)
    return _case('d%d_E%d' % (d, e), d, e, ob, rng)


@functools.lru_cache(maxsize=None)
def periodic(d):
    ob = ac.list_case(d).obs[1]
    assert ob.shift is not None and len(ob.neural_bounds) == 1
    return _case('periodic_d%d' % d, d, len(
        ob.neural_bounds[0].emulator.networks), ob,
        np.random.default_rng(9000 + d))


@functools.lru_cache(maxsize=None)
def reference(kind, *args):
    """Per neural bound of the case ``kind(*args)``: (``ld_scores`` of its
    rows, ``errors`` of the fp64 oracle against them); computed once."""
    c = globals()[kind](*args)
    out = []
    for nb in c.neural:
        ref = ld_scores(nb, c.x, c.shift)
        for a in ref:
            a.setflags(write=False)
        out.append((ref, errors(*oracle_scores(nb, c.x, c.shift), ref)))
    return out


def wraps(case):
    """Per row: the phase shift moves a periodic coordinate across the
    boundary (x + (0.5 - centre) outside [0, 1))."""
    s = case.shift
    v = case.x[:, s.periodic] + (0.5 - s.centers)
    return np.any(np.floor(v) != 0.0, axis=1)


# ---- index lists --------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def index_lists(n=N_ROWS):
    """name -> int64 list into the n rows of a case."""
    rng = np.random.default_rng(5)
    out = dict(identity=np.arange(n), reversed=np.arange(n)[::-1].copy(),
               permutation=rng.permutation(n),
               thrice=np.repeat(np.arange(n), 3),
               one_row=np.full(n, 137), every_third=np.arange(0, n, 3))
    for k in PREFIXES:
        out['prefix_%d' % k] = np.arange(k)
    out = {name: a.astype(np.int64) for name, a in out.items()}
    for a in out.values():
        a.setflags(write=False)
    return out


def long_list(n=N_ROWS):
    """More than 256 passes: workgroups take a second pass, whose rows the
    prefetch finds through the list a pass ahead."""
    return (np.arange(N_LONG) % n).astype(np.int64)


@functools.lru_cache(maxsize=None)
def wide_list(n=N_ROWS):
    """(source, idx): an x of N_WIDE rows, row i a copy of row source[i] of
    the case, and a list of n rows of it that starts at its last row and ends
    at row 0."""
    rng = np.random.default_rng(6)
    source = rng.integers(0, n, size=N_WIDE)
    idx = rng.integers(0, N_WIDE, size=n)
    idx[0], idx[-1] = N_WIDE - 1, 0
    return source.astype(np.int64), idx.astype(np.int64)


# ---- pivot rows and thresholds ------------------------------------------------

def pivot_mask(keep, r2, score, thresholds, m):
    """Rows whose acceptance is decided by the emulator of neural bound ``m``
    alone: kept by the outer union, inside ellipsoid m, and not accepted
    through another neural bound."""
    other = np.zeros(len(keep), dtype=bool)
    for j in range(len(r2)):
        if j != m:
            other |= (r2[j] < 1) & (score[j] > thresholds[j])
    return keep & (r2[m] < 1) & ~other


@functools.lru_cache(maxsize=None)
def oracle_pivots(d):
    """Per neural bound of ``accept_cases.build(d, 3, 2)``: the pivot rows
    among ``accept_cases.proposals(d, 3, 2)``, by the oracle's values."""
    case, p = ac.build(d, 3, 2), ac.proposals(d, 3, 2)
    vals = [oracle_scores(nb, p.x) for nb in case.neural]
    thr = [nb.score_predict_min - 1e-9 for nb in case.neural]
    return [pivot_mask(p.keep, [v[0] for v in vals], [v[1] for v in vals],
                       thr, m) for m in range(len(case.neural))]


def predict_min_for(target):
    """A ``score_predict_min`` whose uploaded threshold, ``float(min) - 1e-9``
    (DeviceBound.thresholds, nb_pack.h), is the double ``target`` exactly.
    Where min and target share a binade, or min lies in the finer one, a step
    of min moves the difference by at most one step of the target's grid, so
    every target is met within a few steps.  Targets in [2^k - 1e-9, 2^k] and
    |target| below about 1e-9 have min on a coarser grid and may be missed:
    ValueError."""
    target = float(target)
    s = target + 1e-9
    for _ in range(8):                      # walk to the nearest from below
        if s - 1e-9 < target:
            break
        s = np.nextafter(s, -np.inf)
    for _ in range(16):
        if float(s) - 1e-9 == target:
            return float(s)
        s = np.nextafter(s, np.inf)
    raise ValueError('no score_predict_min gives the threshold %r' % target)


def with_threshold(ob, m, target):
    """A copy of the ONautilus ``ob`` whose neural bound ``m`` uploads the
    threshold ``target``; everything else is shared."""
    neural = list(ob.neural_bounds)
    neural[m] = copy.copy(neural[m])
    neural[m].score_predict_min = predict_min_for(target)
    return bo.ONautilus.from_parts(ob.outer_bound, neural, shift=ob.shift)


def tile_edge_dims():
    """The first and the last n_dim of every row-tile count in DIMS."""
    return [d for dt in range(1, 9) for d in (16 * (dt - 1) + 1, 16 * dt)]
