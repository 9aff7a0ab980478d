"""Cases and references of the tests of the fused Gaussian-mixture likelihood
(``nb_mixture_loglike``, nautilus_amd/csrc/nb_mixture.hip).  Plain numpy, no
device: shared by test_mixture_cases.py (the table of cases against the
launcher's rules and the reference against scipy and its own bound, on the
CPU), test_mixture_likelihood_gpu.py and test_mixture_sweep_gpu.py (the
kernels against these references).

The kernel is instantiated per DT = ceil(n_dim / 16), per trimming class (from
rem = n_dim mod 16: "full" for rem 9..15 or 0, "small" for rem 1..4, "trimmed"
for rem 5..8) and in a resident and a streamed form (do all records fit the
LDS of a CU?).  ``DIMS`` holds both ends of every class at every DT; the two
component counts of a dimension come from ``device.mixture_launch_shape``."""

import functools

import numpy as np

from nautilus_amd import device

EPS = 2.0**-52
RTOL, ATOL = 1e-11, 1e-8          # the band tests/test_hip_parity.py holds the
#                                   mixture of config 4 to
# z_k ~ OVERLAP_SCALE * N(0, I / D): the distance between two means is about
# sqrt(2) OVERLAP_SCALE standard deviations, so the terms of two components
# differ by about OVERLAP_SCALE^2 +- sqrt(2) OVERLAP_SCALE nats at a draw
OVERLAP_SCALE = 1.0
EXP_RANGE = 700.0                  # exp(-700) = 1e-304 is a normal double


def _random_cov(d, rng, cond=1e3):
    q, _ = np.linalg.qr(rng.normal(size=(d, d)))
    ev = (0.01 + 0.03 * rng.random())**2 * np.logspace(0, -np.log10(cond), d)
    rng.shuffle(ev)
    return (q * ev) @ q.T


def problem(d, k, seed, cond=1e3):
    """Well separated components with covariances of their own."""
    rng = np.random.default_rng(seed)
    means = 0.25 + 0.5 * rng.random((k, d))
    covs = np.stack([_random_cov(d, rng, cond) for _ in range(k)])
    w = rng.random(k) + 0.05
    return means, covs, w / w.sum()


def overlapping(d, k, seed, cond=1e3):
    """One shared covariance L L^T, means mu_0 + L z_k a standard deviation
    or so apart: every point has several terms of similar size."""
    rng = np.random.default_rng(seed)
    cov = _random_cov(d, rng, cond)
    chol = np.linalg.cholesky(cov)
    z = OVERLAP_SCALE * rng.normal(size=(k, d)) / np.sqrt(d)
    means = 0.5 + z @ chol.T
    w = rng.random(k) + 0.05
    return means, cov, w / w.sum()


def draws(means, covs, w, n, rng):
    covs = np.broadcast_to(covs, (len(means),) + covs.shape[-2:])
    which = rng.choice(len(means), size=n, p=w)
    chol = np.linalg.cholesky(covs)
    eps = rng.normal(size=(n, means.shape[1]))
    return means[which] + np.einsum('nij,nj->ni', chol[which], eps)


def points(means, covs, w, seed, n=2000):
    """n draws from the mixture and n uniform points of the cube (the far
    tails: log L down to about -1e6)."""
    rng = np.random.default_rng(seed + 1000)
    return np.vstack([draws(means, covs, w, n, rng),
                      rng.random((n, means.shape[1]))])


def scipy_terms(means, covs, w, x):
    from scipy.stats import multivariate_normal
    covs = np.broadcast_to(covs, (len(means),) + covs.shape[-2:])
    return np.array([np.log(w[i]) + np.atleast_1d(multivariate_normal(
        means[i], covs[i]).logpdf(x)) for i in range(len(means))])


# ---------------------------------------------------------------------------
# the table of cases
# ---------------------------------------------------------------------------
REMS = (1, 4, 5, 8, 9, 15, 16)     # both ends of "small", "trimmed", "full"
DIMS = tuple(16 * (dt - 1) + rem for dt in range(1, 9) for rem in REMS)
N_HALF = 300                       # draws, and as many uniform points


def trim_class(n_dim):
    rem = n_dim % 16
    return 'small' if 1 <= rem <= 4 else 'trimmed' if 5 <= rem <= 8 else 'full'


@functools.lru_cache(maxsize=None)
def largest_resident(n_dim):
    """The largest n_components whose records all fit the LDS, found from
    ``mixture_launch_shape`` (residency is monotone in the count)."""
    lo, hi = 1, device.MIXTURE_MAX_COMPONENTS
    assert device.mixture_launch_shape(n_dim, lo)[4]
    assert not device.mixture_launch_shape(n_dim, hi)[4]
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if device.mixture_launch_shape(n_dim, mid)[4]:
            lo = mid
        else:
            hi = mid
    return lo


def k_resident(n_dim):
    return min(3, largest_resident(n_dim))


def k_streamed(n_dim):
    return largest_resident(n_dim) + 1


CASES = tuple((d, k) for d in DIMS for k in (k_resident(d), k_streamed(d)))


def table_arrays(means, covs, w):
    """(chol_inv, log_coef) by the recipe of ``GaussianMixtureLikelihood``:
    what ``device.MixtureTable`` is handed."""
    from scipy.linalg import solve_triangular
    k, d = means.shape
    covs = np.broadcast_to(covs, (k, d, d))
    chol = np.linalg.cholesky(covs)
    eye = np.eye(d)
    chol_inv = np.stack([np.tril(solve_triangular(c, eye, lower=True))
                         for c in chol])
    log_coef = (np.log(w) - 0.5 * d * np.log(2 * np.pi) -
                np.sum(np.log(np.diagonal(chol, axis1=1, axis2=2)), axis=1))
    return chol_inv, log_coef


def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


@functools.lru_cache(maxsize=None)
def case(d, k, overlap=False, n_half=N_HALF):
    """(means, chol_inv, log_coef, x) of a case, read-only: ``problem`` or
    ``overlapping`` with the seed 100 d + k, n_half draws of the mixture and
    n_half uniform points of the cube."""
    seed = 100 * d + k
    means, covs, w = (overlapping if overlap else problem)(d, k, seed)
    x = points(means, covs, w, seed, n_half)
    chol_inv, log_coef = table_arrays(means, covs, w)
    return _frozen(means, chol_inv, log_coef, x)


# ---------------------------------------------------------------------------
# the reference and its bound
# ---------------------------------------------------------------------------
def fold_bound(k, value):
    """Bound on |device logsumexp - exact logsumexp| of the SAME K fp64 terms,
    for a result near ``value``; u = EPS / 2 is the unit roundoff.

    The kernel keeps (best, sum) with sum = sum_k exp(t_k - best) and, per
    term, either sum += exp(t - best) or sum = sum exp(best - t) + 1.  A step
    errs, relative to the new sum (which is at least 1), by
      * the exponential's own error, 1 ulp <= 2 u;
      * the rounding of its argument a, |a| u, times the share of the new sum
        that the exponential scales: a exp(-a) <= 1 / e for an added term,
        s a exp(-a) / (s exp(-a) + 1) <= 1 + ln s <= 1 + ln K for a rescale
        of a sum s <= K;
      * the rounding of the addition or the fma, u,
    and passes the error it inherits on with a factor of at most 1.  After K
    steps the sum is off by at most K (4 + ln K) u, relatively, and so is
    its logarithm, absolutely.  The logarithm (1 ulp of a value <= ln K) adds
    2 u ln K and the final addition u |value|; another u |value| covers the
    reference's own rounding to fp64.  Terms more than EXP_RANGE below the
    largest one are worth at most K exp(-EXP_RANGE) < K 1e-300 in either
    evaluation."""
    lk = np.log(k)
    return ((0.5 * k * (4 + lk) + lk) * EPS + EPS * np.abs(value) +
            k * 1e-300)


def reference(means, chol_inv, log_coef, x):
    """(values, bound, terms, term_bound): the terms a_k - |W_k (x - mu_k)|^2
    / 2 and their logsumexp in np.longdouble, from the very W_k = chol_inv and
    a_k = log_coef the device table is built from, and bounds on the error of
    an fp64 evaluation in the kernel's order; values and bounds as fp64 of
    shape (n,), terms and term_bound of shape (K, n).

    Per term, with r = x - mu, m = |W| |r| and S = sum_j m_j^2: the centring
    rounds once (u |r_j|), a dot product of at most D non-zero products errs
    by gamma_D m_j (the exact zeros of the padding add no rounding), so y_j is
    off by gamma_(D+1) m_j and y_j^2 by 2 gamma_(D+1) m_j^2; summing the
    squares through at most D / 4 + 6 fused additions adds gamma_(D/4+6) S.
    That is (2.25 D + 8) u S <= 2 (D + 2) EPS S on r^2, half of it on the
    term, and a_k - r^2 / 2 rounds once more: EPS |term| covers that and the
    long double arithmetic of the reference.

    For the fold: logsumexp moves by at most a weighted mean of its terms'
    errors, the weights being each term's share of the sum, so by the largest
    term_bound among the terms within EXP_RANGE of the largest (the others
    weigh less than 1e-300 each); ``fold_bound`` is added for the running sum
    of the kernel."""
    assert np.finfo(np.longdouble).eps < 1e-18
    ld = np.longdouble
    k, d = means.shape
    n = x.shape[0]
    xl = x.astype(ld)
    terms = np.empty((k, n), ld)
    term_bound = np.empty((k, n))
    for i in range(k):
        r = xl - means[i].astype(ld)
        y = r @ chol_inv[i].astype(ld).T
        r2 = np.sum(y * y, axis=1)
        terms[i] = ld(log_coef[i]) - r2 / 2
        mag = np.abs(np.asarray(r, float)) @ np.abs(chol_inv[i]).T
        term_bound[i] = (d + 2) * EPS * np.sum(mag * mag, axis=1) + \
            EPS * np.abs(np.asarray(terms[i], float))
    top = terms.max(axis=0)
    values = top + np.log(np.sum(np.exp(terms - top), axis=0))
    near = np.asarray(top - terms, float) <= EXP_RANGE
    values = np.asarray(values, float)
    bound = np.where(near, term_bound, 0.0).max(axis=0) + fold_bound(k, values)
    return values, bound, terms, term_bound


def clear_labels(terms, term_bound):
    """(label, clear): the index of the largest reference term of every row
    and whether it is decided -- the gap between the two largest terms exceeds
    the sum of their bounds.  With one component every row is clear."""
    k, n = terms.shape
    label = np.argmax(terms, axis=0).astype(np.int32)
    if k == 1:
        return label, np.ones(n, bool)
    order = np.argsort(terms, axis=0)
    first, second = order[-1], order[-2]
    cols = np.arange(n)
    gap = np.asarray(terms[first, cols] - terms[second, cols], float)
    return label, gap > term_bound[first, cols] + term_bound[second, cols]


def twin(means, chol_inv, log_coef, x):
    """(values, terms) in fp64 with BLAS and scipy's logsumexp, from the same
    arrays as ``reference``."""
    from scipy.special import logsumexp
    terms = np.array([log_coef[i] - 0.5 * np.sum(
        ((x - means[i]) @ chol_inv[i].T)**2, axis=1)
        for i in range(len(means))])
    return logsumexp(terms, axis=0), terms


@functools.lru_cache(maxsize=None)
def case_reference(d, k, overlap=False, n_half=N_HALF):
    """``reference`` of ``case``, computed once and read-only."""
    return _frozen(*reference(*case(d, k, overlap, n_half)))


# ---------------------------------------------------------------------------
# several rounds of the loop over points
# ---------------------------------------------------------------------------
# (n_dim, n_components): the resident kernel with 4, 2 and 1 tiles per
# wavefront, the streamed one with each of them and an even and an odd count
# (the record after the last one is fetched on different paths); n_dim mod 16
# in 5..8
ROUND_CASES = ((6, 3), (54, 3), (70, 3),
               (22, 23), (22, 24), (54, 8), (54, 9), (70, 6), (70, 7))
ROUND_BASE = 4099                  # rows of the batch that is tiled


def round_rows(n_dim, n_components):
    """Rows that make three rounds: two full ones -- the second both starts
    from a record 0 fetched during the first and fetches it again -- and a
    last one of one full group of tiles and one group of 5 rows, every other
    wavefront idle."""
    tpw, per_round = device.mixture_launch_shape(n_dim, n_components)[3::2]
    return 2 * per_round + 16 * tpw + 5


def rounds_of(n_dim, n_components, n):
    """[groups of 16 tpw rows per round] of a launch on n rows: the loop of
    nb_mixture.hip restated (a workgroup of 8 wavefronts takes 8 consecutive
    groups, the grid is capped at points_per_round)."""
    tpw, per_round = device.mixture_launch_shape(n_dim, n_components)[3::2]
    group = 16 * tpw
    n_groups = -(-n // group)
    per = per_round // group
    blocks = min(-(-n_groups // 8), per // 8)
    out = []
    for start in range(0, n_groups, blocks * 8):
        out.append(min(blocks * 8, n_groups - start))
    return out
