"""Bounds and rows of the acceptance-route tests, and what the oracle decides
about them.  Plain numpy and the oracle, no device: shared by
test_accept_routes.py (the recipe against its floors, on the CPU) and
test_accept_routes_gpu.py (both acceptance routes and the list evaluation
against these decisions).

``DIMS``: per row-tile count DT = ceil(n_dim / 16) of the evaluation kernels
the dimensions 16 (DT - 1) + 1, + 4, + 5 (both ends of the last row tile with
at most four real rows -- nb_cand.hip's SMALL, taken from DT 2 on -- and the
first dimension behind it), 16 DT - 1 and 16 DT (the last n_dim whose layer 1
has KT1 = DT k-tiles and the first with DT + 1, nb_eval_fast.hip).

The geometry of ``build`` is scaled so that every decision of ``accept`` goes
both ways at every n_dim: members are 1 + 0.7 / n_dim times the neural
ellipsoid (about e^-0.7 of a member's proposals lie inside it whatever n_dim
is), the centres sit 0.7 e from the faces x_0 = 1 and x_{d-1} = 0 with e the
spread of one coordinate of a proposal, and the emulator threshold is the
median score of a probe cloud."""

import functools
import types

import numpy as np

from oracle import bounds_oracle as bo
from oracle import mlp_oracle as mo
from oracle import philox

DIMS = [16 * (dt - 1) + i for dt in range(1, 9) for i in (1, 4, 5, 15, 16)]

N_ROWS, OFFSET = 6000, 10**10 + 7
R2_TOL, SCORE_TOL = 1e-12, 1e-9        # (test_two_stage_large_launch)


def seed_of(d):
    return 31 + d


def instantiation(d):
    """What the dispatch code picks for n_dim = d: nb_eval_fast.hip's
    (DT, KT1) and nb_cand.hip's (DT, SMALL, tiles per wavefront for proposals
    / for lists, STRIP of the proposal kernel)."""
    dt, kt1 = (d + 15) // 16, (d + 1 + 15) // 16
    small = dt > 1 and 1 <= d - 16 * (dt - 1) <= 4
    return dict(fast=(dt, kt1), cand=dict(
        DT=dt, SMALL=small, T_sample=2, T_list=2 if dt <= 5 else 1,
        STRIP_sample=dt != 8))


def _neural(rng, centre, b_mat, seeds, probe_scale, quantile):
    d = len(centre)
    ell = bo.OEllipsoid.from_params(centre, b_mat)
    nb = bo.ONeural()
    nb.outer_bound, nb.n_dim = ell, d
    nb.emulator = mo.Emulator.from_weights(
        rng.normal(size=d) * 0.1, rng.uniform(0.5, 1.5, d),
        [mo.glorot_init(d, s)[:2] for s in seeds])
    probe = centre + (rng.normal(size=(2000, d)) @ b_mat.T) * probe_scale
    nb.score_predict_min = float(np.quantile(
        nb.emulator.predict(ell.transform(probe)), quantile))
    return nb


@functools.lru_cache(maxsize=None)
def build(d, k, m):
    """k outer members and m neural bounds of two Glorot networks each in
    n_dim = d: a namespace with ``outer`` (OUnion), ``ob`` (ONautilus),
    ``neural`` (the ONeural bounds) and ``E``."""
    rng = np.random.default_rng(1000 * d + 10 * k + m)
    e = 0.25 / np.sqrt(d + 2.0)
    centres = 0.5 + 0.15 * e * rng.normal(size=(max(k, m), d))
    centres[:, 0] = 1.0 - 0.7 * e
    centres[:, d - 1] = 0.7 * e
    members, neural = [], []
    for j in range(max(k, m)):
        b_mat = np.tril(rng.normal(size=(d, d)) * 0.01) + np.eye(d) * 0.25
        if j < k:
            members.append(bo.OEllipsoid.from_params(
                centres[j], (1.0 + 0.7 / d) * b_mat))
        if j < m:
            neural.append(_neural(rng, centres[j], b_mat,
                                  [3 * j, 3 * j + 1], 1.0 / np.sqrt(d + 2.0),
                                  0.5))
    outer = bo.OUnion.from_members(members, unit=True)
    return types.SimpleNamespace(
        d=d, k=k, m=m, E=2, outer=outer, neural=neural,
        ob=bo.ONautilus.from_parts(outer, neural))


def decide(case, x, keep):
    """The oracle's decisions about the rows ``x`` of which the outer union
    keeps ``keep`` (union.py:313-319; nautilus.py:212-216, neural.py:115-126):
    ``in_cube``, ``keep``, per neural bound ``inside`` (its ellipsoid) and
    ``reach`` (kept and inside: the rows its emulator has to see), ``accept``,
    ``contains`` (nautilus.py:162-169) and the rows within rounding of a
    decision: ``edge_r2`` per neural bound, ``edge`` (any neural bound's
    ellipsoid or threshold) and ``edge_outer`` (a member's ellipsoid, which
    ``contains`` tests without the stream's overlap count)."""
    n = len(x)
    out = types.SimpleNamespace(
        x=x, keep=keep, in_cube=np.all((x >= 0) & (x < 1), axis=1),
        inside=[], reach=[], edge_r2=[], accept=np.zeros(n, dtype=bool),
        edge=np.zeros(n, dtype=bool), edge_outer=np.zeros(n, dtype=bool))
    for nb in case.neural:
        y = nb.outer_bound.transform(x)
        r2, score = np.sum(y**2, axis=1), nb.emulator.predict(y)
        thr = nb.score_predict_min - 1e-9
        out.inside.append(r2 < 1)
        out.reach.append(keep & (r2 < 1))
        out.edge_r2.append(np.abs(r2 - 1.0) < R2_TOL)
        out.edge |= out.edge_r2[-1] | (np.abs(score - thr) < SCORE_TOL)
        out.accept |= keep & (r2 < 1) & (score > thr)
    for mem in case.outer.bounds:
        r2 = np.sum(mem.transform(x)**2, axis=1)
        out.edge_outer |= np.abs(r2 - 1.0) < R2_TOL
    out.contains = case.ob.contains(x)
    for a in vars(out).values():
        for b in (a if isinstance(a, list) else [a]):
            b.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def proposals(d, k, m):
    """The N_ROWS proposals of ``build(d, k, m)`` on the stream (seed_of(d),
    OFFSET) and the oracle's decisions about them; computed once."""
    case = build(d, k, m)
    x, keep, k_cnt = philox.union_propose(case.outer, seed_of(d), OFFSET,
                                          N_ROWS)
    out = decide(case, x, keep)
    out.k_cnt = k_cnt
    return out


class CubeOuter:
    """An outer union without members: the unit cube alone (what
    ``DeviceBound(n_dim, [], None, True, ...)`` uploads, K = 0)."""

    def __init__(self, n_dim):
        self.n_dim, self.bounds = n_dim, []
        self.cube, self.log_v_all = bo.OCube(n_dim), np.zeros(0)

    def contains(self, x):
        return self.cube.contains(x)


@functools.lru_cache(maxsize=None)
def list_case(d):
    """Nine bounds scattered over the cube and the unit cube behind them (the
    sampler's association list, sampler.py:1002) with the rows to ask about:
    600 around every bound and 2000 uniform ones, permuted.  Bound 1 has a
    periodic shift on features 0 and d - 1, bound 3 no neural bound (two
    members), bound 4 a neural bound without emulator, bound 5 a member with
    cube dimensions (box limits; d > 1), bound 7 no member at all.  Returns a
    namespace: ``obs``, ``x``, ``inside`` (the oracle's ``contains`` of every
    bound, one row each) and ``edge``."""
    rng = np.random.default_rng(17 * d + 9)
    obs, clouds = [], []
    for j in range(9):
        centre = rng.uniform(0.15, 0.85, size=d)
        b_mat = np.tril(rng.normal(size=(d, d)) * 0.004) + np.eye(d) * 0.09
        shift = None
        if j == 1:
            shift = bo.OPhaseShift.from_params(
                np.unique([0, d - 1]), rng.uniform(0.0, 1.0, size=min(d, 2)))
        members = [bo.OEllipsoid.from_params(centre, 1.05 * b_mat)]
        if j == 3:
            members.append(bo.OEllipsoid.from_params(
                centre + 0.05 / np.sqrt(d), 1.05 * b_mat))
        if j == 5 and d > 1:
            free = np.ones(d, dtype=bool)
            free[[1, d - 2]] = False
            members = [bo.OMixture.from_params(
                ~free, bo.OEllipsoid.from_params(
                    centre[free], 1.05 * b_mat[np.ix_(free, free)]))]
        outer = (CubeOuter(d) if j == 7 else
                 bo.OUnion.from_members(members, unit=True))
        neural = []
        if j != 3:
            nb = _neural(rng, centre, b_mat, [2 * j, 2 * j + 1],
                         0.7 / np.sqrt(d), 0.3)
            if j == 4:
                nb.emulator, nb.score_predict_min = None, 0.0
            neural.append(nb)
        obs.append(bo.ONautilus.from_parts(outer, neural, shift=shift))
        # (radii 0.6 to 1.2 of the neural ellipsoid in high dimensions: on
        # both sides of its rim and of the member's at 1.05)
        pts = centre + (rng.normal(size=(600, d)) @ b_mat.T) * (
            rng.uniform(0.6, 1.2, size=(600, 1)) / np.sqrt(d))
        if shift is not None:   # in the frame the sampler sees
            pts = shift.transform(pts % 1.0, inverse=True)
        else:                   # (n_dim 1: the cloud is wider than the cube)
            pts = np.clip(pts, 0.0, np.nextafter(1.0, 0.0))
        clouds.append(pts)
    obs.append(bo.OCube(d))
    x = np.vstack(clouds + [rng.random((2000, d))])
    x = x[rng.permutation(len(x))]
    inside = np.array([ob.contains(x) for ob in obs])
    edge = np.zeros(len(x), dtype=bool)
    for ob in obs[:-1]:
        xs = x if ob.shift is None else ob.shift.transform(x)
        for nb in ob.neural_bounds:
            y = nb.outer_bound.transform(xs)
            edge |= np.abs(np.sum(y**2, axis=1) - 1.0) < R2_TOL
            if nb.emulator is not None:
                edge |= np.abs(nb.emulator.predict(y) -
                               (nb.score_predict_min - 1e-9)) < SCORE_TOL
        for mem in ob.outer_bound.bounds:
            ell = getattr(mem, 'ellipsoid', mem)
            cols = ~mem.dim_cube if hasattr(mem, 'dim_cube') else slice(None)
            edge |= np.abs(np.sum(ell.transform(xs[:, cols])**2, axis=1) -
                           1.0) < R2_TOL
    for a in (x, inside, edge):
        a.setflags(write=False)
    return types.SimpleNamespace(d=d, obs=obs, x=x, inside=inside, edge=edge)
