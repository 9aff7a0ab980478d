"""Rows placed on the rim of an ellipsoid, a long double reference of
``r^2 = |B_inv (x - c)|^2`` and a derived bound on what an fp64 kernel may
deviate from it.  Plain numpy and the oracle, no device: shared by
test_rim_cases.py (the recipe against its floors, on the CPU) and
test_rim_gpu.py (every membership kernel's decision on every row).

Why.  A random cloud of 6 000 to 40 000 rows comes no nearer to r^2 = 1 than
1e-6 to 1e-5, so a kernel whose r^2 is off by 1e-7 relative -- a matrix, a
centre or a sum in single precision -- flips none of its decisions.  The rows
here sit at distances from the rim that start at twice the bound below, where
a correct fp64 kernel cannot flip and a single-precision one flips every
second row (``twin``).

Reference.  ``r2_ref`` evaluates the float64 ``c``, ``B_inv`` (lower triangle,
as ``device.member`` uploads it) and ``x`` in ``np.longdouble``: the inputs
are the kernel's inputs, so what is judged is the kernel's own rounding and
not the conditioning of the problem.

Bound.  With u = 2^-53 and gamma_k = k u / (1 - k u) (Higham, Accuracy and
Stability of Numerical Algorithms, 3.1 and 3.5), for an ellipsoid over d
features:

 1. the kernel rounds x_j - c_j once: d_j (1 + delta), |delta| <= u;
 2. it accumulates y_i = sum_j B_inv_ij d_j over at most d products, fused or
    not, in any order (padding multiplies exact zeros): with 1. the computed
    y_i is off by at most
        e_i = gamma_{d+1} sum_j |B_inv_ij| |x_j - c_j|;
 3. it squares each y_i and sums d of them in any order, fused or not: a dot
    product of the computed y with itself, off by at most gamma_d times the
    sum of the computed squares, each of which is at most (|y_i| + e_i)^2.

 Replacing y_i by the computed value moves sum y_i^2 by at most
 sum_i (2 |y_i| e_i + e_i^2), so
        bound(x) = sum_i (2 |y_i| e_i + e_i^2)
                   + gamma_{d+1} sum_i (|y_i| + e_i)^2.
 It is a function of c, B_inv and x alone; nothing read from a device enters
 it.  For a member whose ellipsoid spans a subset of the features d is the
 number of those features.  ``ld_error`` is the same expression for the
 reference itself (2^-64 per operation, 2 d operations).

Geometry (``geometry``): B lower triangular with diagonal 0.25 and
off-diagonal 0.01 N(0, 1) as in ``accept_cases.build``, the centre
0.5 + 0.01 N(0, 1), B_inv as ``OEllipsoid.from_params`` gives it; the whole
surface r^2 <= 1.01 lies strictly inside the unit cube (asserted).

Ladder (``ladder``): ``bd`` is the largest bound over N_PROBE probe rows at
r^2 = 1; the rungs are r^2 = 1 -+ m bd for m in ``RUNGS`` (at n_dim 128 from
about 2e-13 to about 4e-4).  Each rung and side has PER_RUNG rows: random unit
directions of y and the two rows whose displacement x - c is -+ the longest
semi-axis (-+ sigma_1 times the first left-singular vector of B; y is -+ the
first right-singular one).  Those two are where |x - c| is largest: within
the 1e-9 margin of the bounding-sphere screen of the list kernels
(``radius2``, device.py).  A row is computed as c + B (sqrt(1 -+ m bd) v) and
rescaled three times about c in long double so that ``r2_ref`` of the float64
row hits its target.  The rows of a case are shuffled with a fixed
permutation, so every tile mixes both sides and all rungs.

A row with |r2_ref - 1| <= bound(x) is *undecided* and would have to be left
out of a comparison; test_rim_cases.py shows that no case has one.

Cases (``Case``: ``name``, ``d``, ``ob`` the oracle bound to upload, ``x`` the
rows in the frame the sampler sees, ``rims`` the rim ellipsoids, and per rim
ellipsoid ``r2`` (long double), ``bound``, ``inside``, ``undecided``; per row
``owner`` (whose ladder), ``rung`` and ``want`` (the side it was placed on)):

 * ``ellipsoid(d)``: the bare ellipsoid;
 * ``union(d, at)``: two members, the rim ellipsoid at position ``at`` and a
   small disjoint one near the corner 0: the overlap count is the decision;
 * ``mixture(d)``, d >= 3: one member whose ellipsoid spans all features but
   1 and d - 2, which are uniform in [0, 1);
 * ``neural(d, m)``: one outer member 1.5 times rim ellipsoid 0, m neural
   bounds with their own rim ellipsoids (the second a shifted copy with its
   own ladder) and two Glorot networks each, the threshold 1.0 below the
   lowest score: bit 1 of ``accept`` is the r^2 decision;
 * ``shifted(d)``: ``neural(d, 1)`` behind a periodic shift on features 0 and
   d - 1; the rows go to the sampler's frame with the oracle's inverse shift,
   come back with its forward shift in float64 (bit-exact against the device,
   test_phase_shift_bit_exact) and are placed and classified after that round
   trip."""

import functools
import types

import numpy as np

import accept_cases as ac
from oracle import bounds_oracle as bo
from oracle import mlp_oracle as mo

L = np.longdouble
U = 2.0**-53
U_LD = 2.0**-64

RUNGS = (2, 4, 16, 2**8, 2**16, 2**24, 2**32)
N_PROBE, PER_RUNG = 512, 64
N_ROWS = 2 * len(RUNGS) * PER_RUNG                      # 896
PREFIXES = (1, 17, 33, 65)

# the dimension tables of the device tests (test_rim_cases.py holds the first
# three against the tests they are taken from)
VALUE_DIMS = (1, 16, 17, 33, 50, 64, 65, 81, 100, 113, 128)
STREAM_EVEN = (2, 16, 18, 20, 36, 52, 56, 64, 66, 68, 80, 84, 90, 96, 100, 112,
               116, 128)
STREAM_ODD = (1, 3, 5, 7, 33, 49, 63, 65, 67, 99, 115, 127)
ACCEPT_DIMS = tuple(ac.DIMS)
# the two lists of the random-row stream tests leave out the full-K and the
# trimmed-K instantiation of most tile counts; ACCEPT_DIMS has them all
STREAM_DIMS = tuple(sorted(set(STREAM_EVEN + STREAM_ODD + ACCEPT_DIMS)))
# one per tile count, every kind of last tile, both parities; not n_dim 1,
# where the shift's own rounding of the one coordinate is the whole bound
SHIFT_DIMS = (5, 20, 33, 63, 68, 85, 111, 128)
RIM_DIMS = tuple(sorted(set(VALUE_DIMS + STREAM_DIMS + SHIFT_DIMS)))
TABLE_DIMS = (3, 20, 50, 128)

TWINS = ('f64', 'binv32', 'c32', 'acc32', 'drop')


def stream_variant(d):
    """What nb_stream.hip launches for n_dim = d: (DT, KL, SMALL, parity of
    the row loads, kernel) -- ``nb_row_dispatch`` (nb_dispatch.h) and
    ``launch_variant`` restated."""
    dt, rem = (d + 15) // 16, d & 15
    full = 2 * ((d + 7) >> 3) == 4 * dt
    kernel = 'pipe2' if 2 <= dt <= 4 else 'pipe1' if 5 <= dt <= 7 else 'plain'
    parity = 'one' if d == 1 else 'odd' if d & 1 else 'even'
    return (dt, 4 * dt if full else 4 * dt - 2,
            not full and 1 <= rem <= 4, parity, kernel)


def gamma(k, u=U):
    return k * u / (1.0 - k * u)


# ---- the reference and the bound ------------------------------------------

def _cols(e, x):
    return x if e.cols is None else x[:, e.cols]


def y_ref(e, x):
    """B_inv (x - c) of the rows ``x`` in long double."""
    return (_cols(e, x).astype(L) - e.c.astype(L)) @ e.B_inv.astype(L).T


def r2_ref(e, x):
    y = y_ref(e, x)
    return np.sum(y * y, axis=1)


def bound(e, x, k=None, u=U):
    """The bound of the module docstring per row, as float64; ``k`` products
    and additions per sum at unit roundoff ``u`` (d + 1 at 2^-53)."""
    g = L(gamma(e.d + 1 if k is None else k, u))
    y = np.abs(y_ref(e, x))
    err = g * (np.abs(_cols(e, x).astype(L) - e.c.astype(L)) @
               np.abs(e.B_inv).astype(L).T)
    out = np.sum(2 * y * err + err * err, axis=1) + \
        g * np.sum((y + err)**2, axis=1)
    return out.astype(np.float64)


def ld_error(e, x):
    """What ``r2_ref`` itself may be off: 2^-64 per operation, at most 2 d
    operations behind any of its numbers."""
    return bound(e, x, k=2 * e.d, u=U_LD)


# ---- geometry ---------------------------------------------------------------

def rim(c, b_mat, cols=None):
    """A rim ellipsoid: ``c``, ``B``, ``B_inv`` as uploaded (lower triangle),
    ``cols`` (the features it spans, None for all) and the oracle's
    ``ell``."""
    ell = bo.OEllipsoid.from_params(c, b_mat)
    e = types.SimpleNamespace(d=len(ell.c), c=ell.c, B=ell.B,
                              B_inv=np.tril(ell.B_inv), cols=cols, ell=ell)
    reach = np.sqrt(1.01) * np.linalg.norm(e.B, axis=1)
    assert np.all(e.c - reach > 0) and np.all(e.c + reach < 1)
    return e


def geometry(d, tag=0):
    rng = np.random.default_rng([d, tag])
    b_mat = np.tril(rng.normal(size=(d, d)) * 0.01) + np.eye(d) * 0.25
    return rim(0.5 + 0.01 * rng.normal(size=d), b_mat), rng


def place(e, v, target, through=None):
    """float64 rows c + B (sqrt(target) v), rescaled three times about c so
    that ``r2_ref`` of the row -- of ``through(row)`` where the kernel sees
    the row through a map -- hits ``target``.  In the ellipsoid's own
    features."""
    own = types.SimpleNamespace(**{**vars(e), 'cols': None})
    t = np.broadcast_to(np.asarray(target, dtype=L), (len(v),))
    cl = e.c.astype(L)
    x = (cl + (np.sqrt(t)[:, None] * v.astype(L)) @ e.B.astype(L).T).astype(
        np.float64)
    for _ in range(3):
        seen = x if through is None else through(x)
        scale = np.sqrt(t / r2_ref(own, seen))
        x = (cl + (x.astype(L) - cl) * scale[:, None]).astype(np.float64)
    return x


def _unit(rng, n, d):
    v = rng.normal(size=(n, d))
    return v / np.linalg.norm(v, axis=1, keepdims=True)


def ladder(e, rng, through=None):
    """(rows, want, rung, bd) of one rim ellipsoid, in its own features and
    in ladder order: ``want`` the side a row was placed on (True: inside),
    ``rung`` its index into RUNGS."""
    own = types.SimpleNamespace(**{**vars(e), 'cols': None})
    bd = float(np.max(bound(own, place(e, _unit(rng, N_PROBE, e.d), 1.0))))
    assert RUNGS[-1] * bd < 0.01
    axis = np.linalg.svd(e.B)[2][0]          # B axis = sigma_1 u_1
    v, target, want, rung = [], [], [], []
    for i, m in enumerate(RUNGS):
        for sign in (-1, 1):
            v += [_unit(rng, PER_RUNG - 2, e.d), axis[None], -axis[None]]
            target += [L(1) + sign * L(m) * L(bd)] * PER_RUNG
            want += [sign < 0] * PER_RUNG
            rung += [i] * PER_RUNG
    x = place(e, np.vstack(v), np.array(target, dtype=L), through)
    return x, np.array(want), np.array(rung), bd


def _case(name, d, ob, rims, parts, e_nets=0, shift=None):
    """``parts``: per ladder (rows in the bound's frame, want, rung, bd)."""
    x = np.vstack([p[0] for p in parts])
    owner = np.repeat(np.arange(len(parts)), [len(p[0]) for p in parts])
    perm = np.random.default_rng(len(x)).permutation(len(x))
    x, owner = x[perm], owner[perm]
    want = np.concatenate([p[1] for p in parts])[perm]
    rung = np.concatenate([p[2] for p in parts])[perm]
    seen = x
    if shift is not None:                 # into the frame the sampler sees
        x = shift.transform(x, inverse=True)
        seen = shift.transform(x)
    assert np.all((x >= 0) & (x < 1))
    out = types.SimpleNamespace(
        name=name, d=d, ob=ob, rims=rims, E=e_nets, shift=shift, x=x,
        seen=seen, owner=owner, want=want, rung=rung,
        bd=[p[3] for p in parts], r2=[], bound=[], inside=[], undecided=[])
    for e in rims:
        r2, b = r2_ref(e, seen), bound(e, seen)
        out.r2.append(r2)
        out.bound.append(b)
        out.inside.append(np.asarray(r2 < 1))
        out.undecided.append(np.asarray(np.abs(r2 - 1) <= b))
    for a in vars(out).values():
        for b in (a if isinstance(a, list) else [a]):
            if isinstance(b, np.ndarray):
                b.setflags(write=False)
    return out


# ---- case builders ----------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _base(d):
    """Rim ellipsoid 0 of n_dim d and its ladder: shared by ``ellipsoid``,
    ``union`` and ``neural``."""
    e, rng = geometry(d)
    return e, ladder(e, rng)


@functools.lru_cache(maxsize=None)
def ellipsoid(d):
    e, part = _base(d)
    return _case('ellipsoid_d%d' % d, d, e.ell, [e], [part])


def far_ellipsoid(d):
    """A small ellipsoid near the corner 0, disjoint from every rim
    ellipsoid's bounding box."""
    return bo.OEllipsoid.from_params(np.full(d, 0.06), np.eye(d) * 0.02)


@functools.lru_cache(maxsize=None)
def union(d, at):
    e, part = _base(d)
    members = [far_ellipsoid(d)]
    members.insert(at, e.ell)
    c = _case('union_d%d_at%d' % (d, at), d,
              bo.OUnion.from_members(members, unit=True), [e], [part])
    assert not np.any(members[1 - at].contains(c.x))
    return c


@functools.lru_cache(maxsize=None)
def mixture(d):
    dim_cube = np.zeros(d, dtype=bool)
    dim_cube[[1, d - 2]] = True
    cols = np.flatnonzero(~dim_cube)
    sub, rng = geometry(len(cols), tag=1)
    xs, want, rung, bd = ladder(sub, rng)
    x = rng.random((len(xs), d))
    x[:, cols] = xs
    e = rim(sub.c, sub.B, cols=cols)
    return _case('mixture_d%d' % d, d, bo.OMixture.from_params(dim_cube, e.ell),
                 [e], [(x, want, rung, bd)])


def _with_emulator(e, seeds, rng, x_all):
    nb = bo.ONeural()
    nb.outer_bound, nb.n_dim = e.ell, e.d
    nb.emulator = mo.Emulator.from_weights(
        rng.normal(size=e.d) * 0.1, rng.uniform(0.5, 1.5, e.d),
        [mo.glorot_init(e.d, s)[:2] for s in seeds])
    nb.score_predict_min = float(
        np.min(nb.emulator.predict(e.ell.transform(x_all)))) - 1.0
    return nb


def _neural(d, m, shift=None):
    e0, part0 = _base(d)
    rng = np.random.default_rng([d, 2, m])
    through = None
    if shift is not None:
        def through(x):
            return shift.transform(shift.transform(x, inverse=True))
        part0 = ladder(e0, rng, through)
    rims, parts = [e0], [part0]
    if m == 2:
        # a copy of ellipsoid 0 moved by 0.2 of its own radius
        e1 = rim(e0.c + e0.B @ (0.2 * _unit(rng, 1, d)[0]), e0.B)
        rims.append(e1)
        parts.append(ladder(e1, rng, through))
    outer = bo.OUnion.from_members(
        [bo.OEllipsoid.from_params(e0.c, 1.5 * e0.B)], unit=True)
    x_all = np.vstack([p[0] for p in parts])
    assert np.all(np.sum(outer.bounds[0].transform(x_all)**2, axis=1) < 0.9)
    neural = [_with_emulator(e, [2 * j, 2 * j + 1], rng, x_all)
              for j, e in enumerate(rims)]
    ob = bo.ONautilus.from_parts(outer, neural, shift=shift)
    name = ('shifted_d%d' % d) if shift is not None else (
        'neural_d%d_m%d' % (d, m))
    return _case(name, d, ob, rims, parts, e_nets=2, shift=shift)


@functools.lru_cache(maxsize=None)
def neural(d, m):
    return _neural(d, m)


@functools.lru_cache(maxsize=None)
def shifted(d):
    # (the boundary of the sampler's frame runs through the ellipsoid's
    # centre, whatever n_dim: rows above it wrap in feature 0, rows below it
    # in feature d - 1)
    c = _base(d)[0].c
    centers = np.array([(1.5 - c[0]) % 1.0, (0.5 - c[d - 1]) % 1.0])
    return _neural(d, 1, bo.OPhaseShift.from_params(
        np.unique([0, d - 1]), centers[:min(d, 2)]))


# ---- twins: what a degraded kernel would decide ------------------------------

def twin(kind):
    """A numpy stand-in ``f(e, x) -> r2`` (float64) for a membership kernel:
    ``f64`` correct, ``binv32`` / ``c32`` with the matrix / the centre rounded
    to fp32, ``acc32`` with r^2 summed in fp32, ``drop`` without the smallest
    entry of B_inv's last row."""
    f32 = np.float32

    def f(e, x):
        c, b_inv = e.c, e.B_inv
        if kind == 'binv32':
            b_inv = b_inv.astype(f32).astype(np.float64)
        elif kind == 'c32':
            c = c.astype(f32).astype(np.float64)
        elif kind == 'drop':
            b_inv = b_inv.copy()
            last = np.abs(b_inv[-1])
            b_inv[-1, np.argmin(np.where(last > 0, last, np.inf))] = 0.0
        y = (_cols(e, x) - c) @ b_inv.T
        if kind == 'acc32':
            return np.sum((y * y).astype(f32), axis=1,
                          dtype=f32).astype(np.float64)
        return np.sum(y * y, axis=1)

    assert kind in TWINS
    return f
