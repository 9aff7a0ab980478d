"""The fused device likelihood of weighted, full-covariance Gaussian mixtures
(``nb_mixture_loglike``, nautilus_amd/csrc/nb_mixture.hip) against its numpy
twin and scipy, and end to end through ``Sampler``.  (Problems and points
come from mixture_cases.py; every instantiation of the kernel is swept in
test_mixture_sweep_gpu.py.)"""

import numpy as np
import pytest

from mixture_cases import (ATOL, RTOL, overlapping, points, problem,
                           scipy_terms)

pytestmark = pytest.mark.gpu

GRID = [(1, 2), (2, 1), (3, 5), (17, 3), (49, 3), (50, 4), (50, 64), (100, 7),
        (127, 2), (128, 16)]


def _cases():
    out = []
    for d, k in GRID:
        out.append(pytest.param(d, k, False, id='%d-%d' % (d, k)))
        if d >= 17:
            out.append(pytest.param(d, k, True, id='%d-%d-overlap' % (d, k)))
    return out


def _like(means, covs, w, labels=False):
    from nautilus_amd import GaussianMixtureLikelihood
    return GaussianMixtureLikelihood(means, covs=covs, weights=w,
                                     labels=labels)


@pytest.mark.parametrize('d, k, overlap', _cases())
def test_values_and_labels(d, k, overlap):
    """log L within rtol 1e-11 / atol 1e-8 of the numpy twin and of scipy;
    the label equals the argmax of the CPU terms wherever the two largest of
    them differ by more than 1e-6 (at most 0.1 % of the points may be left
    out by that rule)."""
    import torch
    from scipy.special import logsumexp
    seed = 100 * d + k
    means, covs, w = (overlapping if overlap else problem)(d, k, seed)
    x = points(means, covs, w, seed)
    like = _like(means, covs, w, labels=True)
    ref, ref_lab = like.numpy(x, labels=True)
    terms = like._terms(x)
    if overlap:
        # of the CPU reference itself: at least half of the draws have a
        # second-largest term within 3 nats of the largest
        top = np.sort(terms[:, :2000], axis=0)
        near = np.mean(top[-1] - top[-2] < 3.0)
        print('share of draws with a second term within 3 nats: %.3f' % near)
        assert near >= 0.5
    out, lab = like(torch.from_numpy(x).cuda())
    assert out.is_cuda and out.dtype == torch.float64 and out.shape == (4000,)
    assert lab.is_cuda and lab.dtype == torch.int32 and lab.shape == (4000,)
    out, lab = out.cpu().numpy(), lab.cpu().numpy()
    sp = logsumexp(scipy_terms(means, covs, w, x), axis=0)
    for name, want in (('numpy twin', ref), ('scipy', sp)):
        err = np.abs(out - want) / (ATOL + RTOL * np.abs(want))
        print('%s: largest error %.3g of the band, log L in [%.4g, %.4g]' % (
            name, err.max(), want.min(), want.max()))
    assert np.allclose(out, ref, rtol=RTOL, atol=ATOL)
    assert np.allclose(out, sp, rtol=RTOL, atol=ATOL)
    if k > 1:
        top = np.sort(terms, axis=0)
        clear = top[-1] - top[-2] > 1e-6
    else:
        clear = np.ones(len(x), bool)
    print('points left out of the label check: %d' % np.sum(~clear))
    assert np.mean(~clear) <= 1e-3
    assert np.array_equal(lab[clear], ref_lab[clear])


@pytest.mark.parametrize('d', [2, 50, 128])
def test_one_component_is_a_gaussian(d):
    import torch
    from nautilus_amd import GaussianLikelihood
    means, covs, w = problem(d, 1, 7 + d)
    x = torch.from_numpy(points(means, covs, w, d)).cuda()
    got = _like(means, covs, None)(x).cpu().numpy()
    want = GaussianLikelihood(means[0], covs[0])(x).cpu().numpy()
    assert np.allclose(got, want, rtol=RTOL, atol=ATOL)


@pytest.mark.parametrize('d', [3, 50, 127])
def test_ragged_batches_bit_for_bit(d):
    """Any slice of a batch, taken at an odd row offset, gives the bits the
    same rows have inside the large batch -- with three components resident
    in LDS (d = 3, 50) and streamed through it (d = 127)."""
    import torch
    means, covs, w = problem(d, 3, 11 * d)
    like = _like(means, covs, w, labels=True)
    big = torch.from_numpy(points(means, covs, w, d)).cuda()
    full, full_lab = like(big)
    for n in (0, 1, 15, 16, 17, 63, 65, 1000):
        for off in (1, 777):
            sub = big[off:off + n]
            if n > 0:                   # a view, not a copy
                assert sub.data_ptr() == big.data_ptr() + off * d * 8
            out, lab = like(sub)
            assert out.shape == (n,) and lab.shape == (n,)
            assert torch.equal(out, full[off:off + n]), (n, off)
            assert torch.equal(lab, full_lab[off:off + n]), (n, off)


def test_one_handle_on_two_streams():
    import torch
    means, covs, w = problem(50, 4, 3)
    like = _like(means, covs, w)
    x = torch.from_numpy(points(means, covs, w, 3)).cuda()
    want = like(x)
    torch.cuda.synchronize()
    outs = []
    for s in (torch.cuda.Stream(), torch.cuda.Stream()):
        with torch.cuda.stream(s):
            outs.append(like(x))
    torch.cuda.synchronize()
    assert like._tables and len(like._tables) == 1
    assert torch.equal(outs[0], want) and torch.equal(outs[1], want)


@pytest.mark.parametrize('d, k', [(3, 5), (50, 4), (100, 7)])
def test_labels_do_not_change_the_values(d, k):
    """label_dev = NULL and non-NULL give identical out."""
    import torch
    means, covs, w = problem(d, k, d + k)
    like = _like(means, covs, w)
    x = torch.from_numpy(points(means, covs, w, d)).cuda()
    table = like._table()
    plain = table.loglike(x)
    both, lab = table.loglike(x, labels=True)
    assert torch.equal(plain, both)
    assert lab.dtype == torch.int32


def test_argument_errors_carry_err_arg():
    from nautilus_amd import _lib, device

    def code(means, chol_inv, log_coef):
        with pytest.raises(_lib.NativeError) as err:
            device.MixtureTable(means, chol_inv, log_coef)
        return err.value.code

    eye = np.eye(3)[None]
    mu = np.full((1, 3), 0.5)
    assert device.MixtureTable(mu, eye, [0.0]).n_components == 1
    assert code(np.zeros((1, 129)), np.eye(129)[None], [0.0]) == _lib.ERR_ARG
    assert code(np.zeros((0, 3)), np.zeros((0, 3, 3)), []) == _lib.ERR_ARG
    assert code(np.zeros((4097, 1)), np.ones((4097, 1, 1)),
                np.zeros(4097)) == _lib.ERR_ARG
    assert code(mu * np.nan, eye, [0.0]) == _lib.ERR_ARG
    assert code(mu, eye, [np.inf]) == _lib.ERR_ARG
    assert code(mu, np.where(eye > 0, np.inf, 0.0), [0.0]) == _lib.ERR_ARG
    bad = eye.copy()
    bad[0, 1, 1] = 0.0                                  # diagonal not positive
    assert code(mu, bad, [0.0]) == _lib.ERR_ARG
    bad = eye.copy()
    bad[0, 0, 2] = 1e-3                                 # above the diagonal
    assert code(mu, bad, [0.0]) == _lib.ERR_ARG
    with pytest.raises(ValueError):
        device.MixtureTable(mu, np.eye(4)[None], [0.0])


def test_numpy_in_numpy_out():
    import torch
    means, covs, w = problem(17, 3, 5)
    x = points(means, covs, w, 5)[::7]
    like = _like(means, covs, w, labels=True)
    out, lab = like(x)
    assert isinstance(out, np.ndarray) and isinstance(lab, np.ndarray)
    assert lab.dtype == np.int32
    t_out, t_lab = like(torch.from_numpy(x).cuda())
    assert np.array_equal(out, t_out.cpu().numpy())
    assert np.array_equal(lab, t_lab.cpu().numpy())
    plain = _like(means, covs, w)(x)
    assert isinstance(plain, np.ndarray) and np.array_equal(plain, out)
    # sigma with weights: Sigma_k = sigma^2 I
    from nautilus_amd import GaussianMixtureLikelihood
    iso = GaussianMixtureLikelihood(means, 0.05, weights=w)
    assert np.allclose(iso(x), iso.numpy(x), rtol=RTOL, atol=ATOL)
    assert np.allclose(iso.covs, 0.05**2 * np.eye(17))


def _three_modes():
    means = np.array([[0.25, 0.25, 0.3, 0.7], [0.75, 0.7, 0.3, 0.3],
                      [0.5, 0.25, 0.75, 0.6]])
    rng = np.random.default_rng(4)
    covs = []
    for _ in range(3):
        q, _ = np.linalg.qr(rng.normal(size=(4, 4)))
        axes = 0.02 + 0.02 * rng.random(4)              # semi-axes 0.02 - 0.04
        covs.append((q * axes**2) @ q.T)
    return means, np.stack(covs), np.array([0.6, 0.3, 0.1])


def _run(like):
    from nautilus_amd import Sampler, unit_prior
    s = Sampler(unit_prior, like, n_dim=4, n_live=1000, n_networks=2,
                vectorized=True, seed=1, n_batch=1000)
    s.run(n_eff=5000, discard_exploration=True)
    return s


def test_sampler_recovers_unequal_mode_weights():
    """Three correlated modes of weight 0.6 / 0.3 / 0.1 well inside the cube
    (every mean at least 6 standard deviations from a face, so the mass
    outside is below 1e-6 and the analytic log Z is 0), with the settings and
    the bands of test_multimodal_mixture_evidence_and_mode_weights.  The
    label of every posterior point travels with it as a blob."""
    means, covs, w = _three_modes()
    like = _like(means, covs, w, labels=True)
    s = _run(like)
    print('log Z = %.4f, n_like = %d' % (s.log_z, s.n_like))
    assert abs(s.log_z) < 0.06
    pts, log_w, _, blobs = s.posterior(return_blobs=True)
    share = np.array([np.exp(log_w)[blobs == k].sum() for k in range(3)])
    print('posterior weight per label:', share)
    assert np.allclose(share, w, atol=0.04)
    assert np.array_equal(blobs, like.numpy(pts, labels=True)[1])
    again = _run(_like(means, covs, w, labels=True))
    assert again.log_z == s.log_z and again.n_like == s.n_like
