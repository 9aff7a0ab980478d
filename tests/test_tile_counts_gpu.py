"""The kernels that build the bounds, at every tile count they are compiled
for.

``nb_mvee.hip`` (Khachiyan sweeps, moments, quadratic forms, whitening),
``nb_transform.hip`` and ``nb_gmm.hip`` are instantiated once per number of
16-wide tiles: ``ceil((n_dim + 1) / 16)`` = 1..9 for kernels that work on the
augmented rows q = (x, 1), ``ceil(n_dim / 16)`` = 1..8 for kernels that work
on plain rows.  Every count is other code (register arrays, LDS layouts and
job lists sized by it), so every test here walks one of the two tables below
-- the first and the last n_dim of every count, plus an odd interior one of
the two augmented counts that the workload dimensions (3, 20, 50, 100, 128)
never reach -- and crosses it with the row counts at which the kernel's
workgroups and row tiles change.  The inputs are well conditioned throughout:
this is about coverage, not about hard numerics.

References are numpy (``np.longdouble`` where the band comes from the
reference's own float64 error), ``khachiyan_weights_numpy`` and the oracle's
``OEllipsoid``.  The table test at the top needs no device."""

import numpy as np
import pytest

from helpers import upload, khachiyan_weights_numpy

AUG_DIMS = [1, 15, 16, 31, 32, 39, 47, 48, 63, 64, 79, 80, 87, 95, 96, 111,
            112, 127, 128]
PLAIN_DIMS = [1, 3, 16, 17, 32, 33, 48, 49, 64, 65, 80, 81, 96, 97, 112, 113,
              128]
AUG_DIMS_2 = [d for d in AUG_DIMS if d >= 2]
# the augmented counts no test ran before this table existed
AUG_COUNTS_NEW = (3, 6)
MAX_DIM = 128


def aug_tiles(n_dim):
    return (n_dim + 1 + 15) // 16


def plain_tiles(n_dim):
    return (n_dim + 15) // 16


def test_tables_reach_every_tile_count():
    """Fails when someone trims a table: every count is reached, both ends of
    every count's range are present, and the two counts outside the workload
    dimensions keep an odd n_dim strictly inside their range."""
    for dims, tiles, counts in ((AUG_DIMS, aug_tiles, range(1, 10)),
                                (PLAIN_DIMS, plain_tiles, range(1, 9))):
        assert all(1 <= d <= MAX_DIM for d in dims)
        assert {tiles(d) for d in dims} == set(counts)
        for count in counts:
            span = [d for d in range(1, MAX_DIM + 1) if tiles(d) == count]
            assert span == list(range(span[0], span[-1] + 1))
            if len(span) > 1:
                assert span[0] in dims and span[-1] in dims, (count, span)
    for count in AUG_COUNTS_NEW:
        inside = [d for d in AUG_DIMS if aug_tiles(d) == count and
                  aug_tiles(d - 1) == count and aug_tiles(d + 1) == count]
        assert any(d % 2 == 1 for d in inside), count


@pytest.fixture(scope='module')
def dev():
    import torch
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    from nautilus_amd import device
    return device


def _cuda(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype=float)).cuda()


def _oracle_ellipsoid(d, rng):
    """The recipe of test_ellipsoid_stream_every_variant."""
    from oracle import bounds_oracle as bo
    b_mat = np.tril(rng.normal(size=(d, d)) * 0.05) + np.eye(d) * 0.5
    return bo.OEllipsoid.from_params(np.full(d, 0.5), b_mat), b_mat


# ---------------------------------------------------------------------------
# nb_ellipsoid_transform: nb_transform_kernel<1..8>
# ---------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize('d', PLAIN_DIMS)
def test_transform_every_tile_count(dev, d):
    """``B_inv (x - c)`` against the oracle (basic.py:340) for 1003 points in
    and around the ellipsoid, and the leading rows alone: the kernel takes 16
    rows per wavefront and four wavefronts per workgroup, and a row's result
    does not depend on which rows share its tile."""
    import torch
    rng = np.random.default_rng(2000 + d)
    ell, b_mat = _oracle_ellipsoid(d, rng)
    b = upload(ell)
    x = 0.5 + (rng.normal(size=(1003, d)) @ b_mat.T) / np.sqrt(d + 2.0)
    want = ell.transform(x)
    r2 = np.sum(want**2, axis=-1)
    assert 0.05 < np.mean(r2 < 1) < 0.98
    xt = _cuda(x)
    full = b.transform(xt)
    assert np.allclose(full.cpu().numpy(), want, rtol=0,
                       atol=1e-11 * np.abs(want).max())
    for k in (1, 15, 16, 17, 63, 64, 65):
        assert torch.equal(b.transform(xt[:k]), full[:k]), k


# ---------------------------------------------------------------------------
# nb_standardize
# ---------------------------------------------------------------------------
def _standardize_reference(x):
    """mean, std and (x - mean) / std of the columns in np.longdouble, and
    per column the band a float64 evaluation is allowed: four times what
    numpy's own float64 evaluation of the same expressions (the literal
    neural.py:74-77) misses the longdouble values by -- the device sums in
    another order -- and no less than the tolerances of
    test_transform_and_standardize (mean: 1e-13 max|x| absolute, std: 1e-13
    relative, standardised points: 1e-11 absolute)."""
    xl = x.astype(np.longdouble)
    mean_l = xl.mean(axis=0)
    std_l = xl.std(axis=0)
    z_l = (xl - mean_l) / std_l
    mean = np.mean(x, axis=0)
    std = np.std(x, axis=0)
    z = (x - mean) / std
    band_mean = np.maximum(4 * np.abs(mean - mean_l),
                           1e-13 * np.abs(x).max())
    band_std = np.maximum(4 * np.abs(std - std_l), 1e-13 * np.abs(std_l))
    band_z = np.maximum(4 * np.abs(z - z_l).max(axis=0), 1e-11)
    return (mean_l, std_l, z_l), (band_mean, band_std, band_z)


def _standardize_ratios(ref, band, mean, std, z=None):
    """Worst error / band of the device's mean, std (and standardised
    points), each over the columns."""
    out = [np.max(np.abs(mean - ref[0]) / band[0]),
           np.max(np.abs(std - ref[1]) / band[1])]
    if z is not None:
        out.append(np.max(np.abs(z - ref[2]).max(axis=0) / band[2]))
    return [float(r) for r in out]


@pytest.mark.gpu
@pytest.mark.parametrize('d', [1, 3, 50, 127, 128])
def test_standardize_off_centre_columns(dev, d):
    """``nb_standardize`` on columns far from zero and on small and ragged
    row counts (the kernel sums with 256 threads).  Every third column has
    mean 1e6 and unit spread -- there a mean that is off by an ulp of ITSELF
    moves the standardised coordinates by 1e-10 -- the others are
    ellipsoid-frame coordinates as in test_transform_and_standardize."""
    rng = np.random.default_rng(3000 + d)
    ell, _ = _oracle_ellipsoid(d, rng)
    for n in (2, 255, 256, 257, 1003):
        x = ell.transform(rng.random((n, d)))
        heavy = x[:, 0::3]
        x[:, 0::3] = 1e6 + rng.normal(size=heavy.shape)
        ref, band = _standardize_reference(x)
        mean, scale, xs = dev.standardize(_cuda(x))
        ratios = _standardize_ratios(ref, band, mean.cpu().numpy(),
                                     scale.cpu().numpy(), xs.cpu().numpy())
        print('standardize d=%d n=%d: worst error / band: mean %.3f, std '
              '%.3f, points %.3f' % (d, n, *ratios))
        assert max(ratios) <= 1.0, (d, n, ratios)


# ---------------------------------------------------------------------------
# nb_weighted_moments (nb_moments_kernel<1..9>), nb_quadform_max (sweep mode 1)
# ---------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize('d', AUG_DIMS)
def test_moments_and_quadform_every_tile_count(dev, d):
    """The data and tolerances of test_weighted_moments_and_quadform at row
    counts around one 16-row tile and around the 512 points of a workgroup.
    With n <= n_dim the moment matrix is singular, so the quadratic form is
    taken with a fixed symmetric positive definite matrix there."""
    rng = np.random.default_rng(4000 + d)
    m = d + 1
    a = rng.normal(size=(m, 2 * m))
    p_fixed = a @ a.T / (2 * m) + np.eye(m)
    p_fixed = 0.5 * (p_fixed + p_fixed.T)
    for n in (1, 15, 16, 17, 511, 512, 513, 1500):
        x = rng.normal(size=(n, d)) * 0.3 + 0.1
        w = rng.random(n)
        q = np.hstack([x, np.ones((n, 1))])
        s = dev.weighted_moments(x, _cuda(w), 0.5).cpu().numpy()
        ref = 0.5 * (q * w[:, None]).T @ q
        assert np.allclose(s, ref, rtol=1e-12, atol=1e-12), n
        s1 = dev.weighted_moments(x).cpu().numpy()
        assert np.allclose(s1, q.T @ q, rtol=1e-12, atol=1e-12), n
        if n > d:
            p = np.linalg.inv(q.T @ q / n)
            p = 0.5 * (p + p.T)
        else:
            p = p_fixed
        g = np.einsum('ij,jk,ik->i', q, p, q)
        got = float(dev.quadform_max(x, p).cpu()[0])
        assert abs(got - g.max()) < 1e-10 * g.max(), n


# ---------------------------------------------------------------------------
# nb_whiten: nb_standardize, nb_moments_kernel, nb_whiten_factor_kernel,
# nb_transform_kernel
# ---------------------------------------------------------------------------
def _white_residual(xw):
    xl = xw.astype(np.longdouble)
    return float(np.abs(xl.T @ xl / len(xl) - np.eye(xl.shape[1])).max())


@pytest.mark.gpu
@pytest.mark.parametrize('d', AUG_DIMS_2)
def test_whiten_every_tile_count(dev, d):
    """``device.whiten`` on its own.  W is lower triangular with a positive
    diagonal, and with that shape W C W^T = I has one solution (the inverse
    Cholesky factor of the correlation matrix C), so W is judged by how white
    the points come out -- against what ``inv(cholesky(C))`` in numpy achieves
    on the same standardised points; the device eliminates in another order
    and applies W on the matrix cores, hence eight times that."""
    rng = np.random.default_rng(5000 + d)
    for n in (2 * d + 5, 1500):
        mix = np.eye(d) + 0.1 * rng.normal(size=(d, d)) / np.sqrt(d)
        x = (rng.normal(size=(n, d)) * rng.uniform(0.5, 2.0, size=d) +
             0.3) @ mix.T
        # a condition on the inputs, not a result
        assert np.linalg.cond(np.corrcoef(x, rowvar=False)) < 100, n
        xw, stats = dev.whiten(_cuda(x))
        xw = xw.cpu().numpy()
        stats = stats.cpu().numpy()
        mean, sd = stats[:d], stats[d:2 * d]
        w = stats[2 * d:].reshape(d, d)
        ref, band = _standardize_reference(x)
        ratios = _standardize_ratios(ref, band, mean, sd)
        assert np.all(np.triu(w, 1) == 0.0) and np.all(np.diag(w) > 0.0)
        xs = (x - mean) / sd
        want = xs @ w.T
        assert np.allclose(xw, want, rtol=0, atol=1e-11 * np.abs(want).max())
        w_ref = np.linalg.inv(np.linalg.cholesky(xs.T @ xs / n))
        res_ref = _white_residual(xs @ w_ref.T)
        res = _white_residual(xw)
        print('whiten d=%d n=%d: worst error / band: mean %.3f, sd %.3f; '
              'max|xw^T xw / n - I| = %.3e, numpy %.3e, residual / band '
              '%.3f' % (d, n, *ratios, res, res_ref, res / (8 * res_ref)))
        assert max(ratios) <= 1.0, (n, ratios)
        assert res <= 8 * res_ref, (n, res, res_ref)


# ---------------------------------------------------------------------------
# Khachiyan: nb_mvee_sweep_kernel<1..9, 20 | 32>
# ---------------------------------------------------------------------------
def _cloud(rng, n, d):
    """The point sets of test_mvee_kernel_shapes."""
    return rng.normal(size=(n, d)) * rng.uniform(0.5, 2.0, size=d) + 0.3


def _check_weights(u, pts, n_batch, what):
    u_h = khachiyan_weights_numpy(pts, n_batch=n_batch)
    assert abs(u.sum() - 1.0) < 1e-12, what
    assert np.allclose(u, u_h, rtol=0, atol=1e-8), what


@pytest.mark.gpu
@pytest.mark.parametrize('d', AUG_DIMS_2)
def test_khachiyan_every_tile_count(dev, d):
    """``nb_mvee_weights`` against the numpy iteration with one workgroup
    (n_dim + 2 points), a ragged second one and, where 389 points are more
    than n_dim, four with a short last one."""
    rng = np.random.default_rng(6000 + d)
    for n in (d + 2, 2 * d + 5, 389):
        if n <= d:
            continue
        pts = _cloud(rng, n, d)
        _check_weights(dev.mvee_weights(pts).cpu().numpy(), pts, 20, (d, n))


@pytest.mark.gpu
def test_khachiyan_wide_candidate_lists(dev):
    """``n_batch = 32`` (32 candidates per sweep, NSC = 32) at one n_dim per
    tile count.  The LDS layout grows with both, and the launcher refuses
    what exceeds 160 KB with ERR_UNSUPPORTED before it launches a sweep: a
    case is either served correctly or refused, the refused ones are the
    upper end of the tile counts, everything up to n_dim 50 is served, and a
    refusal leaves the default fit of the same points intact."""
    from nautilus_amd import _lib
    dims = (7, 20, 39, 50, 70, 87, 100, 120, 128)
    assert [aug_tiles(d) for d in dims] == list(range(1, 10))
    rng = np.random.default_rng(6500)
    served = []
    for d in dims:
        pts = _cloud(rng, 300, d)
        try:
            u = dev.mvee_weights(pts, n_batch=32).cpu().numpy()
        except _lib.NativeError as err:
            assert err.code == _lib.ERR_UNSUPPORTED, (d, err)
            served.append(False)
            _check_weights(dev.mvee_weights(pts).cpu().numpy(), pts, 20,
                           (d, 'after the refusal'))
            continue
        served.append(True)
        _check_weights(u, pts, 32, d)
    refused = [d for d, ok in zip(dims, served) if not ok]
    print('n_batch = 32 refused at n_dim %s (tile counts %s)' % (
        refused, [aug_tiles(d) for d in refused]))
    assert served == sorted(served, reverse=True), served
    assert all(ok for d, ok in zip(dims, served) if d <= 50), served


@pytest.mark.gpu
@pytest.mark.parametrize('d', [80, 87, 95])
def test_mvee_six_tiles(dev, d):
    """``geometry.mvee`` (whitening, sweeps, moments and the largest quadratic
    form in one fit) at the tile count of n_dim 80..95: every point inside,
    one on the surface (basic.py:236-239), A A^-1 = 1."""
    from nautilus_amd import geometry
    rng = np.random.default_rng(6600 + d)
    pts = rng.normal(size=(700, d)) * rng.uniform(0.2, 3.0, size=d)
    c, a, a_inv = geometry.mvee(pts)
    r2 = np.einsum('ij,jk,ik->i', pts - c, a, pts - c)
    assert abs(r2.max() - 1.0) < 1e-12
    assert np.allclose(a @ a_inv, np.eye(d), atol=1e-9)


@pytest.mark.gpu
def test_mvee_batch_equals_single_fits_six_tiles(dev):
    """test_mvee_batch_equals_single_fits at n_dim 87: every set of a batch
    gets exactly the result of a fit of its own."""
    from nautilus_amd import geometry
    rng = np.random.default_rng(6700)
    d = 87
    sets = [rng.normal(size=(n, d)) * rng.uniform(0.2, 3.0, size=d)
            for n in (100, 1000, 333)]
    geometry._ELL_CACHE.clear()
    batch = geometry.mvee_batch(sets)
    for pts, (c, a, a_inv) in zip(sets, batch):
        c1, a1, a_inv1 = geometry.mvee(pts)
        assert np.array_equal(c, c1) and np.array_equal(a, a1)
        assert np.array_equal(a_inv, a_inv1)
        r2 = np.einsum('ij,jk,ik->i', pts - c, a, pts - c)
        assert abs(r2.max() - 1.0) < 1e-12
        assert np.allclose(a @ a_inv, np.eye(d), atol=1e-9)
