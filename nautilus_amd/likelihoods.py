"""Device likelihoods for the BASELINE benchmark problems (SURVEY.md section 8
row A15): callables marked ``device = True`` receive the batch as a cuda
tensor of unit-cube points and return a cuda tensor of log-likelihoods, so the
shell-filling loop never leaves the GPU.  Any other callable handed to
``Sampler`` is evaluated on the host exactly as in the reference.
"""

import numpy as np
import torch

from . import device


def unit_prior(x):
    """Identity prior transform on the unit cube (works on numpy arrays and
    cuda tensors)."""
    return x


unit_prior.device = True


class GaussianLikelihood:
    """Multivariate normal log-density  -1/2 (x-mu)^T Sigma^-1 (x-mu) + const.

    The quadratic form is the same lower-triangular contraction as
    ``Ellipsoid.contains`` (|L^-1 (x - mu)|^2 with Sigma = L L^T) and runs on
    the matrix cores through ``nb_neural_score``."""

    device = True

    def __init__(self, mean, cov, normalised=True):
        mean = np.asarray(mean, float)
        cov = np.atleast_2d(np.asarray(cov, float))
        d = len(mean)
        if cov.shape == (1, 1) and d > 1:
            cov = np.eye(d) * cov[0, 0]
        chol = np.linalg.cholesky(cov)
        self.n_dim = d
        self.mean, self.cov = mean, cov
        self.log_norm = (-0.5 * (d * np.log(2 * np.pi) +
                                 2 * np.sum(np.log(np.diag(chol))))
                         if normalised else 0.0)
        self._chol = chol
        self._dev = None

    def _bound(self):
        if self._dev is None:
            self._dev = device.DeviceBound(
                self.n_dim, [], None, False,
                [dict(ellipsoid=device.member(self.mean, self._chol))])
        return self._dev

    def __call__(self, x):
        r2, _ = self._bound().neural_score(x)
        out = self.log_norm - 0.5 * r2
        return out if isinstance(x, torch.Tensor) else out.cpu().numpy()

    def numpy(self, x):
        """Pure-numpy evaluation (CPU baseline / oracle runs)."""
        y = np.linalg.solve(self._chol, (np.atleast_2d(x) - self.mean).T)
        return self.log_norm - 0.5 * np.sum(y**2, axis=0)

    def __getstate__(self):
        state = dict(self.__dict__)
        state['_dev'] = None
        return state


class _DeviceTables:
    """The device handles of a likelihood, one per device, built on first use
    by the subclass's ``_make_table`` and left behind when it is pickled."""

    def _table(self):
        """The device handle of the current device, built on first use."""
        dev = torch.cuda.current_device()
        if dev not in self._tables:
            self._tables[dev] = self._make_table()
        return self._tables[dev]

    def __getstate__(self):
        state = dict(self.__dict__)
        if '_tables' in state:
            state['_tables'] = {}
        return state


def _numbers(a, p, name, positive):
    """``a`` as P finite numbers that are positive / not negative."""
    a = np.asarray(a, float)
    if a.shape != (p,) or not np.all(np.isfinite(a)) or \
            not np.all(a > 0 if positive else a >= 0):
        raise ValueError('%s must be %d %s' % (
            name, p, 'positive finite numbers' if positive
            else 'finite numbers that are not negative'))
    return a


def _bounded_vector(a, name, n_max, unit):
    """``a`` as a vector of 1 to ``n_max`` numbers."""
    a = np.asarray(a, float)
    if a.ndim != 1 or len(a) < 1:
        raise ValueError('%s must be a vector of at least one number' % name)
    if len(a) > n_max:
        raise ValueError('at most %d %s are supported, not %d' %
                         (n_max, unit, len(a)))
    return a


class _ModelLikelihood(_DeviceTables):
    """A likelihood that runs the user's ``model`` on the batch and then one
    fused kernel on what it returns.  A subclass says how wide the rows of
    every output are (``_widths``), makes its table (``_make_table``) and has
    the pure-numpy ``numpy_from_model``; ``_pair`` is set where the model
    returns a pair of outputs and ``_what`` names them in messages."""

    device = True
    _pair = False
    _what = 'the model output'

    def __init__(self, model):
        if not callable(model):
            raise ValueError('model must be callable')
        self.model = model
        self._tables = {}

    def _check(self, m):
        p = self._widths()[0]
        if m.ndim != 2 or m.shape[1] != p:
            raise ValueError('the model output must have shape (n, %d), not '
                             '%s' % (p, tuple(m.shape)))

    @staticmethod
    def _rows(t, width):
        """``t`` on the device, as it is where its rows can be read in place
        and contiguous otherwise."""
        t = t if t.is_cuda else t.cuda()
        in_place = (width == 1 or t.stride(1) == 1) and \
            (t.shape[0] <= 1 or t.stride(0) >= width)
        return t if in_place else t.contiguous()

    def _loglike(self, *rows):
        return self._table().loglike(*rows)

    def _from_outputs(self, *outputs):
        """``from_model``: float64 cuda tensors in, a cuda tensor out; numpy
        in, numpy out."""
        tensors = isinstance(outputs[0], torch.Tensor)
        if not tensors:
            outputs = [np.asarray(t) for t in outputs]
        for t in outputs:
            if t.dtype != (torch.float64 if tensors else np.float64):
                raise ValueError('%s must be float64, not %s' %
                                 (self._what, t.dtype))
        self._check(*outputs)
        if tensors:
            return self._loglike(*[self._rows(t, width) for t, width in
                                   zip(outputs, self._widths())])
        return self._from_outputs(*[
            torch.from_numpy(np.ascontiguousarray(t)).cuda()
            for t in outputs]).cpu().numpy()

    def _outputs(self, x):
        if self._pair:
            m, w = self.model(x)       # anything but a pair fails to unpack
            return m, w
        return (self.model(x),)

    def __call__(self, x):
        if isinstance(x, torch.Tensor):
            return self.from_model(*self._outputs(x))
        xs = device.as_device_points(x)
        return self.from_model(*self._outputs(xs)).cpu().numpy()

    def numpy(self, x):
        """Pure-numpy twin of a call: the model runs on the CPU."""
        x = np.atleast_2d(np.asarray(x, float))
        return self.numpy_from_model(*[
            t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else t
            for t in self._outputs(torch.from_numpy(x))])


class _PairLikelihood(_ModelLikelihood):
    """A likelihood of P measurements ``data`` with error bars ``sigma`` whose
    model returns a pair: the (n, P) prediction and a second output, which
    ``_second`` names in messages and whose rows are ``_width`` wide."""

    _pair = True
    _what = property(lambda self: 'the model output and the ' + self._second)

    def _set_data(self, data, n_max):
        """``data`` and ``n_data``; returns P."""
        data = _bounded_vector(data, 'data', n_max, 'data points')
        if not np.all(np.isfinite(data)):
            raise ValueError('data must be finite')
        self.data = data.copy()
        self.n_data = len(data)
        return self.n_data

    def _set_sigma(self, sigma, normalised):
        """``sigma``, ``_sigma2`` and ``log_norm``, once ``n_data`` is set."""
        p = self.n_data
        if sigma is None:
            self.sigma = np.zeros(p)
        else:
            self.sigma = _numbers(sigma, p, 'sigma', False).copy()
        with np.errstate(over='ignore'):
            self._sigma2 = self.sigma * self.sigma
        if not np.all(np.isfinite(self._sigma2)):
            raise ValueError('sigma is too large: sigma^2 is not finite')
        self.log_norm = -0.5 * p * np.log(2 * np.pi) if normalised else 0.0

    def _widths(self):
        return self.n_data, self._width

    def _second_shape(self, n):
        return n, self._width

    def _check(self, m, w):
        super()._check(m)
        if w.ndim != 2 or tuple(w.shape) != (m.shape[0], self._width):
            raise ValueError('the %s must have shape %s, not %s' % (
                self._second, self._second_shape(m.shape[0]),
                tuple(w.shape)))

    def _same_kind(self, m, w):
        if isinstance(m, torch.Tensor) != isinstance(w, torch.Tensor):
            raise ValueError('%s must both be torch tensors or both numpy '
                             'arrays' % self._what)


class GaussianMixtureLikelihood(_DeviceTables):
    """Mixture of Gaussians  log sum_k w_k N(x; mu_k, Sigma_k).

    ``GaussianMixtureLikelihood(means, sigma)`` is the equal-weight isotropic
    mixture of BASELINE config 4, a composition of ``GaussianLikelihood``
    parts.  Any of ``covs`` ((D, D) shared or (K, D, D)), ``weights`` (K
    positive numbers, normalised by their sum) or ``labels=True`` selects the
    fused kernel ``nb_mixture_loglike`` instead: one launch that reads every
    point once, for unequal weights and correlated components.  With
    ``labels=True`` a call returns ``(log_l, label)``, ``label`` being the
    int32 index of the largest term (the component a point belongs to);
    ``Sampler`` carries it through as a blob.

    A non-finite entry in row i of the points makes ``log_l[i]`` of the fused
    kernel NaN -- or -inf, where an infinite entry meets no exact zero of any
    inverse Cholesky factor or of its padding -- never a finite value or +inf,
    and changes no bit of the value or the label of any other row; the label
    of such a row means nothing."""

    device = True

    def __init__(self, means, sigma=None, *, covs=None, weights=None,
                 labels=False):
        self.means = np.atleast_2d(np.asarray(means, float))
        if (sigma is None) == (covs is None):
            raise ValueError('exactly one of sigma and covs must be given')
        self.sigma = None if sigma is None else float(sigma)
        k, d = self.means.shape
        self.n_components, self.n_dim = k, d
        self.labels = bool(labels)
        self.fused = covs is not None or weights is not None or self.labels
        if not self.fused:
            self.parts = [GaussianLikelihood(m, np.eye(d) * sigma**2)
                          for m in self.means]
            self.covs = np.broadcast_to(np.eye(d) * self.sigma**2,
                                        (k, d, d)).copy()
            self.weights = np.full(k, 1.0 / k)
            return
        self.parts = None
        if not np.all(np.isfinite(self.means)):
            raise ValueError('means must be finite')
        if covs is None:
            if not (np.isfinite(self.sigma) and self.sigma > 0):
                raise ValueError('sigma must be positive and finite')
            covs = np.eye(d) * self.sigma**2
        covs = np.asarray(covs, float)
        if covs.shape == (d, d):
            covs = np.broadcast_to(covs, (k, d, d))
        if covs.shape != (k, d, d):
            raise ValueError('covs must have shape (%d, %d) or (%d, %d, %d), '
                             'not %s' % (d, d, k, d, d, covs.shape))
        self.covs = covs.copy()
        if weights is None:
            weights = np.full(k, 1.0)
        weights = _numbers(weights, k, 'weights', True)
        self.weights = weights / np.sum(weights)
        self._chol = np.empty((k, d, d))
        for i in range(k):
            try:
                if not np.all(np.isfinite(self.covs[i])):
                    raise np.linalg.LinAlgError('not finite')
                self._chol[i] = np.linalg.cholesky(self.covs[i])
            except np.linalg.LinAlgError:
                raise ValueError('the covariance of component %d is not '
                                 'positive definite' % i) from None
        self._log_coef = (np.log(self.weights) - 0.5 * d * np.log(2 * np.pi) -
                          np.sum(np.log(np.diagonal(self._chol, axis1=1,
                                                    axis2=2)), axis=1))
        self._tables = {}

    def _make_table(self):
        from scipy.linalg import solve_triangular
        eye = np.eye(self.n_dim)
        chol_inv = np.stack([np.tril(solve_triangular(c, eye, lower=True))
                             for c in self._chol])
        return device.MixtureTable(self.means, chol_inv, self._log_coef)

    def __call__(self, x):
        if not self.fused:
            xs = device.as_device_points(x)
            stack = torch.stack([p(xs) for p in self.parts])
            out = torch.logsumexp(stack, dim=0) - np.log(len(self.parts))
            return out if isinstance(x, torch.Tensor) else out.cpu().numpy()
        res = self._table().loglike(x, labels=self.labels)
        if isinstance(x, torch.Tensor):
            return res
        if self.labels:
            return res[0].cpu().numpy(), res[1].cpu().numpy()
        return res.cpu().numpy()

    def numpy(self, x, labels=False):
        """Pure-numpy evaluation (CPU baseline / oracle runs / tests); with
        ``labels`` also the index of the largest term."""
        from scipy.special import logsumexp
        if not self.fused:
            parts = [p.numpy(x) for p in self.parts]
            out = logsumexp(parts, axis=0) - np.log(len(self.parts))
            if labels:
                return out, np.argmax(parts, axis=0).astype(np.int32)
            return out
        terms = self._terms(x)
        out = logsumexp(terms, axis=0)
        if labels:
            return out, np.argmax(terms, axis=0).astype(np.int32)
        return out

    def _terms(self, x):
        """(K, n) array of log w_k N(x_i; mu_k, Sigma_k)."""
        from scipy.linalg import solve_triangular
        x = np.atleast_2d(np.asarray(x, float))
        terms = np.empty((self.n_components, x.shape[0]))
        for i in range(self.n_components):
            y = solve_triangular(self._chol[i], (x - self.means[i]).T,
                                 lower=True)
            terms[i] = self._log_coef[i] - 0.5 * np.sum(y**2, axis=0)
        return terms


N_DATA_MAX = 4096                  # NB_CHI2_MAX_DATA of include/nautilus_hip.h


class GaussianDataLikelihood(_ModelLikelihood):
    """Gaussian likelihood of a data vector:  log L(theta) = log_norm -
    1/2 (m(theta) - d)^T C^-1 (m(theta) - d).

    ``model`` takes the (n, n_dim) batch of points as a torch tensor and
    returns the (n, P) float64 predictions on the same device; ``data`` holds
    the P measurements; exactly one of ``cov`` ((P, P), symmetric positive
    definite) and ``sigma`` (P positive numbers, a diagonal covariance) is
    given.  P is at most 4096.  ``log_norm = -1/2 (P log 2 pi + log det C)``,
    or 0 with ``normalised=False``.

    A call evaluates the model and then runs the fused kernel
    ``nb_chi2_loglike`` -- one launch on the current stream that multiplies by
    the triangle of W = L^-1 (C = L L^T) only and never stores the n x P
    product.  ``from_model`` is the second half alone; it reads a cuda tensor
    whose rows are strided (``stride(1) == 1``, ``stride(0) >= P``, such as a
    column slice of a wider tensor) in place and copies anything else to
    contiguous.  ``numpy`` / ``numpy_from_model`` are the pure-numpy twins.

    A non-finite entry in row i of the model output makes ``out[i]`` NaN and
    changes no bit of any other row."""

    def __init__(self, model, data, *, cov=None, sigma=None, normalised=True):
        super().__init__(model)
        data = _bounded_vector(data, 'data', N_DATA_MAX, 'data points')
        if not np.all(np.isfinite(data)):
            raise ValueError('data must be finite')
        if (cov is None) == (sigma is None):
            raise ValueError('exactly one of cov and sigma must be given')
        self.data = data.copy()
        self.n_data = p = len(data)
        self.cov = self.sigma = self._chol = None
        if sigma is not None:
            sigma = _numbers(sigma, p, 'sigma', True)
            self.sigma = sigma.copy()
            log_det = 2.0 * np.sum(np.log(sigma))
        else:
            cov = np.asarray(cov, float)
            if cov.shape != (p, p):
                raise ValueError('cov must have shape (%d, %d), not %s' %
                                 (p, p, cov.shape))
            try:
                if not np.all(np.isfinite(cov)) or \
                        not np.allclose(cov, cov.T, rtol=1e-10, atol=0.0):
                    raise np.linalg.LinAlgError('not symmetric and finite')
                self._chol = np.linalg.cholesky(cov)
            except np.linalg.LinAlgError:
                raise ValueError('cov is not positive definite (symmetric, '
                                 'finite, every eigenvalue positive)') \
                    from None
            self.cov = cov.copy()
            log_det = 2.0 * np.sum(np.log(np.diag(self._chol)))
        self.log_norm = (-0.5 * (p * np.log(2 * np.pi) + log_det)
                         if normalised else 0.0)

    def _make_table(self):
        if self.sigma is not None:
            return device.Chi2Table(self.data, inv_sigma=1.0 / self.sigma,
                                    log_norm=self.log_norm)
        from scipy.linalg import solve_triangular
        chol_inv = np.tril(solve_triangular(
            self._chol, np.eye(self.n_data), lower=True))
        return device.Chi2Table(self.data, chol_inv=chol_inv,
                                log_norm=self.log_norm)

    def _widths(self):
        return (self.n_data,)

    def from_model(self, m):
        """log L of the rows of an (n, P) float64 model output: a cuda tensor
        in, a cuda tensor out; numpy in, numpy out."""
        return self._from_outputs(m)

    def numpy_from_model(self, m):
        """Pure-numpy evaluation of an (n, P) model output (CPU baseline /
        oracle runs / tests)."""
        m = np.asarray(m, float)
        self._check(m)
        r = m - self.data
        if self.sigma is not None:
            y = r / self.sigma
        else:
            from scipy.linalg import solve_triangular
            finite = np.where(np.isfinite(r), r, 0.0)
            y = solve_triangular(self._chol, finite.T, lower=True,
                                 check_finite=False).T
        out = self.log_norm - 0.5 * np.sum(y**2, axis=1)
        out[~np.all(np.isfinite(r), axis=1)] = np.nan
        return out


N_COUNTS_MAX = 1 << 20             # NB_POISSON_MAX_DATA of nautilus_hip.h
N_SOURCE_MAX = 1 << 20             # NB_FOLD_MAX_SOURCE
N_RESPONSE_MAX = 1 << 24           # NB_FOLD_MAX_RESPONSE, doubles when packed


def poisson_log_const(counts):
    """Per bin  k log k - k - lgamma(k + 1)  (0 for k = 0), the part of the
    Poisson log-probability that the deviance leaves out.  From k = 16 on it
    is the Stirling series -1/2 log(2 pi k) - 1/(12 k) + 1/(360 k^3) -
    1/(1260 k^5) + ..., not the difference of two numbers of size k log k;
    the series runs to the k^-11 term, which leaves less than 2e-18 at
    k = 16.  Below 16 the direct expression is formed in ``np.longdouble``
    (lgamma by the same series after shifting the argument past 16) and
    rounded once: within 0.2 eps max(1, |C|) where long double is the 80-bit
    type (x86-64 Linux).  Where ``np.longdouble`` is float64 the same code
    runs in float64 and errs by up to about 4 eps |C| for k between 2 and
    16 (a RuntimeWarning says so once per call)."""
    k = np.asarray(counts, float)
    out = np.zeros(k.shape)

    def series(x):
        # sum_n B_2n / (2n (2n - 1) x^(2n - 1)), n = 1 .. 6
        y = 1 / (x * x)
        return (1 / x) * (1 / x.dtype.type(12) + y * (
            -1 / x.dtype.type(360) + y * (1 / x.dtype.type(1260) + y * (
                -1 / x.dtype.type(1680) + y * (1 / x.dtype.type(1188) - y * (
                    x.dtype.type(691) / x.dtype.type(360360)))))))

    big = k >= 16
    kb = k[big]
    out[big] = -0.5 * np.log(2 * np.pi * kb) - series(kb)
    small = (k > 0) & ~big
    if np.any(small) and np.finfo(np.longdouble).eps >= np.finfo(float).eps:
        import warnings
        warnings.warn('np.longdouble is float64 here: poisson_log_const is '
                      'accurate to about 4 eps |C| only below k = 16',
                      RuntimeWarning)
    ks = k[small].astype(np.longdouble)
    # lgamma(k + 1) = stirling(k + 17) - sum_{i = 1 .. 16} log(k + i)
    z = ks + 17
    two_pi = 2 * np.arccos(np.longdouble(-1))
    lg = (z - 0.5) * np.log(z) - z + 0.5 * np.log(two_pi) + series(z)
    for i in range(1, 17):
        lg = lg - np.log(ks + i)
    out[small] = (ks * np.log(ks) - ks - lg).astype(float)
    return out


class PoissonDataLikelihood(_ModelLikelihood):
    """Poisson likelihood of counts in bins:  log L(theta) = sum_j log
    Poisson(k_j | mu_j(theta)),  mu_j = exposure_j m_j(theta) + background_j.

    ``model`` takes the (n, n_dim) batch of points as a torch tensor and
    returns the (n, P) float64 predictions on the same device; ``counts``
    holds the P observed counts k_j >= 0 (they need not be integers, as in an
    Asimov data set; a positive count must have a finite reciprocal, and
    mu / k must stay below the float64 maximum -- with counts under 1e-290 a
    finite mu can overflow it and the row is NaN); ``exposure`` (P positive numbers, default 1) and
    ``background`` (P numbers >= 0, default 0) map the model onto expected
    counts.  P is at most 2^20.

    The sum is evaluated in the deviance form

        log L = log_const - sum_j D(mu_j, k_j),       D(mu, 0) = mu,
        D(mu, k) = k (t - lg),   t = (mu - k) (1 / k),
                   lg = log1p(t) if |t| < 1/2 else log(mu (1 / k)),

    whose terms are all >= 0: nothing cancels, unlike in k log mu - mu for
    large counts.  ``log_const = sum_j [k_j log k_j - k_j - lgamma(k_j + 1)]``
    (``poisson_log_const``) makes the result the sum of
    ``scipy.stats.poisson.logpmf(k, mu)``; with ``normalised=False`` it is 0
    and the result is -1/2 of Cash's C statistic (Cash 1979).

    A call evaluates the model and then runs the fused kernel
    ``nb_poisson_loglike`` -- one streaming launch on the current stream that
    reads every model row once.  ``from_model`` is the second half alone; it
    reads a cuda tensor whose rows are strided (``stride(1) == 1``,
    ``stride(0) >= P``, such as a column slice of a wider tensor) in place
    and copies anything else to contiguous.  ``numpy`` / ``numpy_from_model``
    are the pure-numpy twins, ``numpy_deviance`` the matrix of the D.

    In row i,  mu = 0 in a bin with k > 0 makes ``out[i]`` -inf (mu = 0 with
    k = 0 contributes 0); a negative, NaN or infinite mu makes it NaN, also
    next to a -inf bin.  Neither changes a bit of any other row.

    With ``response`` = a (P, K) matrix R the model lives in a source space:
    it returns (n, K) values s (fluxes in K true-energy bins, amplitudes of K
    templates) and  mu_j = exposure_j sum_k R_jk s_k + background_j.  R may
    hold any finite values; ceil16(P) ceil16(K) is at most 2^24 (4096 x 4096,
    or 2^20 x 16).  The fused kernel ``nb_fold_poisson_loglike`` forms the mu
    on the fp64 matrix cores and feeds them straight into the deviance, so
    the (n, P) expected counts are never stored; ``from_model`` then takes
    (n, K) under the same layout rules, ``n_source`` is K, and the numpy
    twins fold with ``s @ R.T`` first.  A NaN or infinite source value makes
    its row NaN, also where the column of R it meets is all zeros."""

    def __init__(self, model, counts, *, exposure=None, background=None,
                 normalised=True, response=None):
        super().__init__(model)
        counts = _bounded_vector(counts, 'counts', N_COUNTS_MAX, 'bins')
        if not np.all(np.isfinite(counts)) or not np.all(counts >= 0):
            raise ValueError('counts must be finite and not negative')
        with np.errstate(divide='ignore', over='ignore'):
            if not np.all(np.isfinite(1.0 / counts[counts > 0])):
                raise ValueError('a positive count is too small: 1 / k is '
                                 'not finite')
        self.counts = counts.copy()
        self.n_data = p = len(counts)
        if exposure is None:
            self.exposure = np.ones(p)
        else:
            self.exposure = _numbers(exposure, p, 'exposure', True).copy()
        if background is None:
            self.background = np.zeros(p)
        else:
            self.background = _numbers(background, p, 'background',
                                       False).copy()
        if response is None:
            self.response = None
            self.n_source = p
        else:
            response = np.asarray(response, float)
            if response.ndim != 2 or response.shape[0] != p or \
                    response.shape[1] < 1:
                raise ValueError('response must have shape (%d, K) with K >= '
                                 '1, not %s' % (p, response.shape))
            k_src = response.shape[1]
            if k_src > N_SOURCE_MAX or \
                    16 * ((p + 15) // 16) * 16 * ((k_src + 15) // 16) > \
                    N_RESPONSE_MAX:
                raise ValueError(
                    'the response is too large: K <= %d and ceil16(P) '
                    'ceil16(K) <= %d are supported, not %s' %
                    (N_SOURCE_MAX, N_RESPONSE_MAX, response.shape))
            if not np.all(np.isfinite(response)):
                raise ValueError('response must be finite')
            self.response = response.copy()
            self.n_source = k_src
        # 1 / k as the device table holds it: 0 where k = 0
        self._inv_counts = np.zeros(p)
        np.divide(1.0, counts, out=self._inv_counts, where=counts > 0)
        self.log_const = (float(np.sum(poisson_log_const(counts)))
                          if normalised else 0.0)
        if not np.isfinite(self.log_const):
            raise ValueError('counts are too large: log_const is not finite')

    def _make_table(self):
        if self.response is None:
            return device.PoissonTable(
                self.counts, self.exposure, self.background,
                log_const=self.log_const)
        return device.FoldedPoissonTable(
            self.counts, self.response, self.exposure, self.background,
            log_const=self.log_const)

    def _widths(self):
        return (self.n_source,)

    def from_model(self, m):
        """log L of the rows of an (n, P) float64 model output ((n, K) with a
        response): a cuda tensor in, a cuda tensor out; numpy in, numpy
        out."""
        return self._from_outputs(m)

    def numpy_deviance(self, m):
        """The (n, P) terms D(mu_ij, k_j) of an (n, P) model output ((n, K)
        with a response) in pure numpy, by the formulas of the class
        docstring: +inf where mu = 0 and k > 0, NaN where mu is negative, NaN
        or infinite."""
        m = np.asarray(m, float)
        self._check(m)
        k, ik = self.counts, self._inv_counts
        with np.errstate(all='ignore'):
            if self.response is not None:
                m = m @ self.response.T
            mu = self.exposure * m + self.background
            fin = (mu >= 0) & (mu < np.inf)
            pos = np.broadcast_to(k > 0, mu.shape)
            live = fin & (mu > 0) & pos
            t = np.where(live, (mu - k) * ik, 0.0)
            small = np.abs(t) < 0.5
            lg = np.where(small, np.log1p(np.where(small, t, 0.0)),
                          np.log(np.where(small, 1.0, mu * ik)))
            d = np.where(pos, k * (t - lg), mu)
        d[fin & (mu == 0) & pos] = np.inf
        d[~fin] = np.nan
        return d

    def numpy_from_model(self, m):
        """Pure-numpy evaluation of an (n, P) model output, (n, K) with a
        response (CPU baseline / oracle runs / tests)."""
        d = self.numpy_deviance(m)
        flagged = ~np.isfinite(d)
        out = self.log_const - np.sum(np.where(flagged, 0.0, d), axis=1)
        out[np.any(np.isinf(d), axis=1)] = -np.inf
        out[np.any(np.isnan(d), axis=1)] = np.nan
        return out


N_NOISE_MAX = 1 << 20              # NB_NOISE_MAX_DATA of nautilus_hip.h


class GaussianNoiseLikelihood(_PairLikelihood):
    """Gaussian likelihood of independent measurements whose error bars carry
    free parameters:

        log L(theta) = log_norm - 1/2 sum_j [ (m_j - d_j)^2 / v_j + log v_j ].

    The variance v depends on the point, so the ``log v`` term always stays;
    ``log_norm = -(P/2) log 2 pi``, or 0 with ``normalised=False``.

    ``data`` holds the P finite measurements, P at most 2^20; ``sigma`` the P
    quoted error bars, finite and >= 0 (``None`` = all zero; zero is legal
    because the model noise may carry the whole variance).  ``model`` takes
    the (n, n_dim) batch of points as a torch tensor and returns a pair
    ``(m, w)`` of float64 tensors on the same device: ``m`` the (n, P)
    predictions and ``w`` the noise,

      noise='row'   w is (n, 3) with columns (c, a, f):
                    v_ij = c_i sigma_j^2 + a_i + f_i m_ij^2 -- an error
                    inflation factor, a jitter variance added in quadrature
                    and a fractional model variance, one triple per point;
      noise='full'  w is (n, P):  v_ij = sigma_j^2 + w_ij, any variance model.

    A call evaluates the model and then runs the fused kernel
    ``nb_noise_loglike`` -- one streaming launch on the current stream that
    reads every row once and takes no log per element (the mantissas of the v
    are multiplied and their exponents added).  ``from_model`` is the second
    half alone; it reads a cuda tensor whose rows are strided
    (``stride(1) == 1``, ``stride(0)`` at least the width, such as a column
    slice of a wider tensor) in place and copies anything else to contiguous,
    separately for ``m`` and ``w``.  ``numpy`` / ``numpy_from_model`` are the
    pure-numpy twins, ``numpy_terms`` the two matrices of the summands.

    Row i is NaN when any m_ij is not finite or any v_ij is not in (0, +inf):
    zero, negative, NaN or infinite, whichever coefficient caused it.  That
    changes no bit of any other row.  The signs of the single coefficients do
    not matter as long as v > 0."""

    _second = 'noise'

    def __init__(self, model, data, sigma=None, *, noise='row',
                 normalised=True):
        super().__init__(model)
        if noise not in ('row', 'full'):
            raise ValueError("noise must be 'row' or 'full', not %r" %
                             (noise,))
        self.noise = noise
        self._set_data(data, N_NOISE_MAX)
        self._set_sigma(sigma, normalised)

    @property
    def _width(self):
        return 3 if self.noise == 'row' else self.n_data

    def _make_table(self):
        return device.NoiseTable(self.data, self._sigma2,
                                 log_norm=self.log_norm)

    def _loglike(self, m, w):
        return self._table().loglike(
            m, w, device.NOISE_ROW if self.noise == 'row'
            else device.NOISE_FULL)

    def from_model(self, m, w):
        """log L of the rows of an (n, P) float64 model output and its noise
        ((n, 3) or (n, P)): cuda tensors in, a cuda tensor out; numpy in,
        numpy out."""
        self._same_kind(m, w)
        return self._from_outputs(m, w)

    def numpy_variance(self, m, w):
        """The (n, P) variances v_ij of an (n, P) model output and its noise,
        in pure numpy and as they come: a v outside (0, +inf) is not marked
        here."""
        m, w = np.asarray(m, float), np.asarray(w, float)
        self._check(m, w)
        with np.errstate(all='ignore'):
            if self.noise == 'row':
                return w[:, 0:1] * self._sigma2 + w[:, 1:2] + \
                    w[:, 2:3] * (m * m)
            return self._sigma2 + w

    def numpy_terms(self, m, w):
        """The (n, P) pair (chi^2 terms (m - d)^2 / v, log v) in pure numpy;
        both are NaN where m is not finite or v is not in (0, +inf)."""
        m = np.asarray(m, float)
        v = self.numpy_variance(m, w)
        with np.errstate(all='ignore'):
            good = np.isfinite(m) & (v > 0) & (v < np.inf)
            vg = np.where(good, v, 1.0)
            r = np.where(good, m, 0.0) - self.data
            chi = np.where(good, r * r / vg, np.nan)
            log_v = np.where(good, np.log(vg), np.nan)
        return chi, log_v

    def numpy_from_model(self, m, w):
        """Pure-numpy evaluation of an (n, P) model output and its noise (CPU
        baseline / oracle runs / tests)."""
        chi, log_v = self.numpy_terms(m, w)
        bad = np.isnan(chi)
        out = self.log_norm - 0.5 * np.sum(np.where(bad, 0.0, chi + log_v),
                                           axis=1)
        out[np.any(bad, axis=1)] = np.nan
        return out


class GaussianOutlierLikelihood(_PairLikelihood):
    """Gaussian likelihood of independent measurements some of which are
    outliers -- the two-component mixture per measurement of Hogg, Bovy &
    Lang (2010): a measurement is either good, with the model's mean and
    variance, or bad, drawn from a broad Gaussian whose fraction, mean and
    width are free parameters:

        log L(theta) = log_norm + sum_j log[
            (1 - p) v_j^-1/2 exp(-(m_j - d_j)^2 / (2 v_j))
            +    p  u_j^-1/2 exp(-(d_j - b)^2 / (2 u_j)) ],

    ``log_norm = -(P/2) log 2 pi``, or 0 with ``normalised=False``.

    ``data`` holds the P finite measurements, P at most 2^20; ``sigma`` the P
    quoted error bars, finite and >= 0 (``None`` = all zero).  ``model`` takes
    the (n, n_dim) batch of points as a torch tensor and returns a pair
    ``(m, w)`` of float64 tensors on the same device: ``m`` the (n, P)
    predictions and ``w`` (n, 6) with columns (c, a, f, p, b, s),

      v_ij = c_i sigma_j^2 + a_i + f_i m_ij^2   the inlier variance, the
                                                expression of
                                                ``GaussianNoiseLikelihood``
                                                with noise='row';
      u_ij = sigma_j^2 + s_i                    the outlier variance;
      p_i in [0, 1]                             the outlier fraction;
      b_i                                       the outlier mean.

    A call evaluates the model and then runs the fused kernel
    ``nb_outlier_loglike`` -- one streaming launch on the current stream that
    reads every row once, takes no log and one exp per element and never
    underflows: the component with the larger exponent is taken out of the
    sum, so a measurement hundreds of sigma away from the model costs what
    the outlier component says and not ``-inf``.  ``p = 0`` and ``p = 1`` give
    the one-component value.  ``from_model`` is the second half alone, with
    the layout rules of ``GaussianNoiseLikelihood.from_model``.  ``numpy`` /
    ``numpy_from_model`` are the pure-numpy twins, ``numpy_terms`` the two
    weighted log densities of every measurement and
    ``numpy_responsibilities`` the posterior probability that a measurement
    is an outlier (host only; for posterior samples).

    Row i is NaN when any m_ij or b_i is not finite, any v_ij or u_ij is not
    in (0, +inf), or p_i is outside [0, 1], NaN included.  That changes no bit
    of any other row."""

    _second = 'mixture'
    _width = device.OUTLIER_WIDTH

    def __init__(self, model, data, sigma=None, *, normalised=True):
        super().__init__(model)
        self._set_data(data, N_NOISE_MAX)
        self._set_sigma(sigma, normalised)

    def _make_table(self):
        return device.NoiseTable(self.data, self._sigma2,
                                 log_norm=self.log_norm)

    def _loglike(self, m, w):
        return self._table().outlier_loglike(m, w)

    def from_model(self, m, w):
        """log L of the rows of an (n, P) float64 model output and its (n, 6)
        mixture coefficients: cuda tensors in, a cuda tensor out; numpy in,
        numpy out."""
        self._same_kind(m, w)
        return self._from_outputs(m, w)

    def _parts(self, m, w):
        """(e1, e2, A1, A2, bad) of an (n, P) model output and its mixture in
        pure numpy: the two exponents, the two amplitudes (1 - p) v^-1/2 and
        p u^-1/2, and where an element makes its row NaN; there the other
        four are those of a standard normal at its mean."""
        m, w = np.asarray(m, float), np.asarray(w, float)
        self._check(m, w)
        c, a, f, p, b, s = (w[:, i:i + 1] for i in range(6))
        with np.errstate(all='ignore'):
            v = c * self._sigma2 + a + f * (m * m)
            u = self._sigma2 + s
            bad = ~(np.isfinite(m) & (v > 0) & (v < np.inf) & (u > 0) &
                    (u < np.inf) & (p >= 0) & (p <= 1) & np.isfinite(b))
            yv = 1.0 / np.sqrt(np.where(bad, 1.0, v))
            yu = 1.0 / np.sqrt(np.where(bad, 1.0, u))
            r1 = np.where(bad, 0.0, m - self.data)
            r2 = np.where(bad, 0.0, self.data - b)
            e1 = -0.5 * ((r1 * r1) * (yv * yv))
            e2 = -0.5 * ((r2 * r2) * (yu * yu))
            a1 = np.where(bad, 1.0, (1.0 - p) * yv)
            a2 = np.where(bad, 0.0, p * yu)
        return e1, e2, a1, a2, bad

    def numpy_terms(self, m, w):
        """The (n, P) pair of weighted log densities log[(1 - p) v^-1/2] -
        (m - d)^2 / (2 v) and log[p u^-1/2] - (d - b)^2 / (2 u) in pure
        numpy, without the constant: ``-inf`` where the weight is zero, NaN
        where the element makes its row NaN."""
        e1, e2, a1, a2, bad = self._parts(m, w)
        with np.errstate(divide='ignore'):
            l1 = np.where(bad, np.nan, e1 + np.log(a1))
            l2 = np.where(bad, np.nan, e2 + np.log(a2))
        return l1, l2

    def numpy_responsibilities(self, m, w):
        """The (n, P) posterior probabilities that measurement j is an outlier
        at point i, p N(d | b, u) / [(1 - p) N(d | m, v) + p N(d | b, u)], in
        pure numpy (host only: made for posterior samples); NaN where the
        element makes its row NaN."""
        l1, l2 = self.numpy_terms(m, w)
        with np.errstate(all='ignore'):
            return np.exp(l2 - np.logaddexp(l1, l2))

    def numpy_from_model(self, m, w):
        """Pure-numpy evaluation of an (n, P) model output and its mixture
        (CPU baseline / oracle runs / tests), in the arithmetic of the
        kernel: log q = e_hi + log(A_hi + A_lo exp(e_lo - e_hi))."""
        e1, e2, a1, a2, bad = self._parts(m, w)
        with np.errstate(all='ignore'):
            one = (a2 == 0.0) | ((a1 != 0.0) & (e1 >= e2))
            e_hi, e_lo = np.where(one, e1, e2), np.where(one, e2, e1)
            a_hi, a_lo = np.where(one, a1, a2), np.where(one, a2, a1)
            big_b = a_hi + a_lo * np.exp(np.minimum(e_lo - e_hi, 0.0))
            out = self.log_norm + np.sum(e_hi + np.log(big_b), axis=1)
        out[np.any(bad, axis=1)] = np.nan
        return out


N_GP_MAX = 128                     # NB_GP_MAX_DATA of nautilus_hip.h
GP_KERNELS = ('sqexp', 'exp', 'matern32', 'matern52')


def gp_correlation(kernel, r):
    """The isotropic correlation function rho(r) of ``kernel`` at r = D / l
    >= 0, with the operations and their order of ``gp_rho`` in nb_gp.hip;
    numpy float64 or ``np.longdouble`` in, the same type out."""
    r = np.asarray(r)
    ty = r.dtype.type
    r = np.minimum(r, ty(1e4))         # rho is 0 in float64 long before
    if kernel == 'sqexp':
        return np.exp(-ty(0.5) * (r * r))
    if kernel == 'exp':
        return np.exp(-r)
    if kernel == 'matern32':
        u = np.sqrt(ty(3)) * r
        return (1 + u) * np.exp(-u)
    if kernel == 'matern52':
        u = np.sqrt(ty(5)) * r
        return ((1 + u) + (u * u) * (1 / ty(3))) * np.exp(-u)
    raise ValueError('kernel must be one of %s, not %r' %
                     (', '.join(map(repr, GP_KERNELS)), kernel))


class GaussianProcessLikelihood(_PairLikelihood):
    """Gaussian-process likelihood of P correlated measurements whose full
    covariance depends on the point:

        log L(theta) = log_norm - 1/2 [ r^T K^-1 r + log det K ],
        r = m(theta) - data.

    ``log_norm = -(P/2) log 2 pi``, or 0 with ``normalised=False``; the
    determinant depends on the point and always stays.

    ``t`` holds the P input locations, (P,) or (P, d), of which the Euclidean
    distances D_jk = |t_j - t_k| alone are kept; ``data`` the P finite
    measurements, P at most 128; ``sigma`` the P fixed error bars, finite and
    >= 0 (``None`` = all zero).  ``model`` takes the (n, n_dim) batch of
    points as a torch tensor and returns a pair of float64 tensors on the
    same device: ``m`` the (n, P) mean prediction and

      cov='hyper'  ``h`` (n, 3) with columns (a, l, s) -- signal variance,
                   length scale and a jitter variance added in quadrature:
                   K_jk = a rho(D_jk / l) + delta_jk (sigma_j^2 + s), where
                   rho is ``kernel``, a function of r = D / l:
                     'sqexp'     exp(-r^2 / 2)
                     'exp'       exp(-r)
                     'matern32'  (1 + sqrt(3) r) exp(-sqrt(3) r)
                     'matern52'  (1 + sqrt(5) r + 5 r^2 / 3) exp(-sqrt(5) r)
                   and the diagonal is a + sigma_j^2 + s exactly;
      cov='full'   ``C`` (n, P, P):  K = C + diag(sigma^2), any covariance
                   model; only the lower triangle (k <= j) of every C is
                   read, ``t`` may be ``None`` and ``kernel`` is ignored.

    A call evaluates the model and then runs the fused kernel
    ``nb_gp_loglike`` -- one launch on the current stream with one workgroup
    per point, which builds K in on-chip memory, factorises it on the fp64
    matrix cores and never stores it, so that the (n, P, P) tensor of hyper
    mode never exists.  ``from_model`` is the second half alone; it reads a
    cuda tensor whose rows are strided (``stride(1) == 1``, ``stride(0)`` at
    least the width, such as a column slice of a wider tensor; for ``C`` every
    matrix contiguous and the matrices any distance >= P^2 apart) in place
    and copies anything else to contiguous, separately for the two outputs.
    ``numpy`` / ``numpy_from_model`` are the pure-numpy twins (LAPACK's
    Cholesky, one matrix at a time), ``numpy_covariance`` the K they
    factorise.

    Row i is NaN when any m_ij is not finite; when a is negative or not
    finite (a = 0 is legal: white noise only), l is outside (0, +inf) or s is
    negative or not finite; when the lower triangle of C holds a non-finite
    entry; or when K is not positive definite to working precision (a pivot
    of the factorisation outside (0, +inf)).  That changes no bit of any
    other row."""

    _second = 'covariance input'

    def __init__(self, model, t, data, sigma=None, *, kernel='sqexp',
                 cov='hyper', normalised=True):
        super().__init__(model)
        if cov not in ('hyper', 'full'):
            raise ValueError("cov must be 'hyper' or 'full', not %r" % (cov,))
        self.cov = cov
        if kernel not in GP_KERNELS:
            raise ValueError('kernel must be one of %s, not %r' %
                             (', '.join(map(repr, GP_KERNELS)), kernel))
        self.kernel = kernel
        p = self._set_data(data, N_GP_MAX)
        if t is None:
            if cov == 'hyper':
                raise ValueError("cov='hyper' needs the input locations t")
            self.t = self.dist = None
        else:
            t = np.asarray(t, float)
            if t.ndim not in (1, 2) or t.shape[0] != p or \
                    (t.ndim == 2 and t.shape[1] < 1):
                raise ValueError('t must have shape (%d,) or (%d, d), not %s'
                                 % (p, p, t.shape))
            if not np.all(np.isfinite(t)):
                raise ValueError('t must be finite')
            self.t = t.copy()
            tt = t.reshape(p, -1)
            with np.errstate(over='ignore'):
                self.dist = np.sqrt(np.sum(
                    (tt[:, None, :] - tt[None, :, :])**2, axis=2))
            if not np.all(np.isfinite(self.dist)):
                raise ValueError('t is too spread out: a distance is not '
                                 'finite')
        self._set_sigma(sigma, normalised)

    @property
    def _width(self):
        return 3 if self.cov == 'hyper' else self.n_data * self.n_data

    def _make_table(self):
        return device.GPTable(self.data, self._sigma2, self.dist,
                              kernel=self.kernel, log_norm=self.log_norm)

    def _loglike(self, m, c):
        return self._table().loglike(
            m, c, device.GP_HYPER if self.cov == 'hyper' else device.GP_FULL)

    def _second_shape(self, n):
        if self.cov == 'hyper':
            return (n, 3)
        return (n, self.n_data, self.n_data)

    def _flat(self, c):
        """The (n, P, P) covariances as (n, P^2) rows: a view where every
        matrix is contiguous, a copy otherwise."""
        p = self.n_data
        if self.cov == 'hyper' or c.ndim != 3 or \
                tuple(c.shape[1:]) != (p, p):
            return c
        n = c.shape[0]
        if not isinstance(c, torch.Tensor):
            return np.ascontiguousarray(c).reshape(n, p * p)
        if n > 0 and (p == 1 or (c.stride(2) == 1 and c.stride(1) == p)):
            return c.as_strided((n, p * p), (c.stride(0), 1))
        return c.contiguous().view(n, p * p)

    def from_model(self, m, c):
        """log L of the rows of an (n, P) float64 model output and its
        covariance input ((n, 3) or (n, P, P)): cuda tensors in, a cuda
        tensor out; numpy in, numpy out."""
        self._same_kind(m, c)
        if not isinstance(c, torch.Tensor):
            c = np.asarray(c)
        if self.cov == 'full' and (c.ndim != 3 or tuple(c.shape[1:]) !=
                                   (self.n_data, self.n_data)):
            raise ValueError('the covariance input must have shape %s, not %s'
                             % (self._second_shape(len(m)), tuple(c.shape)))
        return self._from_outputs(m, self._flat(c))

    def numpy_covariance(self, m, c):
        """The (n, P, P) covariances K of an (n, P) model output and its
        covariance input in pure numpy, as they come (symmetric, built from
        the lower triangle; nothing is marked here)."""
        m, c = np.asarray(m, float), np.asarray(c, float)
        self._check(m, self._flat(c))
        n, p = m.shape
        diag = np.arange(p)
        with np.errstate(all='ignore'):
            if self.cov == 'hyper':
                a, l, s = (c[:, i, None, None] for i in range(3))
                k = a * gp_correlation(self.kernel, self.dist * (1.0 / l))
                k[:, diag, diag] = a[:, 0] + (self._sigma2 + s[:, 0])
                return k
            low = np.tril(c.reshape(n, p, p))
            k = low + np.transpose(np.tril(low, -1), (0, 2, 1))
            k[:, diag, diag] += self._sigma2
            return k

    def numpy_from_model(self, m, c):
        """Pure-numpy evaluation of an (n, P) model output and its covariance
        input (CPU baseline / oracle runs / tests)."""
        from scipy.linalg import solve_triangular
        m, c = np.asarray(m, float), np.asarray(c, float)
        k = self.numpy_covariance(m, c)
        n, p = m.shape
        low = np.tril(np.ones((p, p), bool))
        good = np.all(np.isfinite(m), axis=1) & \
            np.all(np.isfinite(k[:, low]), axis=1)
        if self.cov == 'hyper':
            a, l, s = c.T
            with np.errstate(invalid='ignore'):
                good &= (a >= 0) & (a < np.inf) & (l > 0) & (l < np.inf) & \
                    (s >= 0) & (s < np.inf)
        out = np.full(n, np.nan)
        rows = np.flatnonzero(good)
        try:
            chol = dict(zip(rows, np.linalg.cholesky(k[rows])))
        except np.linalg.LinAlgError:
            chol = {}
            for i in rows:
                try:
                    chol[i] = np.linalg.cholesky(k[i])
                except np.linalg.LinAlgError:
                    pass
        for i, low_i in chol.items():
            d = np.diag(low_i)
            if not np.all((d > 0) & (d < np.inf)):
                continue
            y = solve_triangular(low_i, m[i] - self.data, lower=True,
                                 check_finite=False)
            out[i] = self.log_norm - 0.5 * (np.sum(y * y) +
                                            2.0 * np.sum(np.log(d)))
        return out


N_GPS_MAX = 1 << 20                # NB_GPS_MAX_DATA of nautilus_hip.h
GPS_KERNELS = ('exp', 'matern32', 'matern52', 'sho')
GPS_CAP = 1e4                      # of dt / l, the cap of gp_correlation
GPS_STATES = {'exp': 1, 'matern32': 2, 'matern52': 3, 'sho': 2}
GPS_MAX_TERMS = 3                  # NB_GPS_MAX_TERMS of nautilus_hip.h
GPS_MAX_STATES = 6                 # NB_GPS_MAX_STATES


def sho_correlation(r, q):
    """rho(r; q) = exp(-r / (2 q)) [cos(eta r) + sin(eta r) / (2 eta q)], eta
    = sqrt(1 - 1 / (4 q^2)): the correlation of the underdamped oscillator of
    quality factor q > 1/2 at r = |dt| / l >= 0, capped as ``gp_correlation``
    caps r; numpy float64 or ``np.longdouble`` in, the same type out."""
    r = np.asarray(r)
    ty = r.dtype.type
    r = np.minimum(r, ty(GPS_CAP))
    w = 1 / (2 * np.asarray(q, r.dtype))
    eta = np.sqrt(1 - w * w)
    return np.exp(-(r * w)) * (np.cos(eta * r) + np.sin(eta * r) / eta * w)


def sum_in_order(terms):
    """The terms added from the first on, as the kernels add them."""
    total = None
    for term in terms:
        total = term if total is None else total + term
    return total


class GaussianProcessSeriesLikelihood(_PairLikelihood):
    """Gaussian-process likelihood of an ordered series of P correlated
    measurements, evaluated as a filter in O(P) per point:

        log L(theta) = log_norm - 1/2 [ r^T K^-1 r + log det K ],
        r = m(theta) - data,
        K_jk = a rho(|t_j - t_k| / l) + delta_jk (sigma_j^2 + s).

    This is the likelihood of ``GaussianProcessLikelihood(cov='hyper')`` for
    a one-dimensional ``t`` and the kernels whose process is a linear
    stochastic differential equation with a finite state -- which lifts the
    limit on P from 128 to 2^20.  ``log_norm = -(P/2) log 2 pi``, or 0 with
    ``normalised=False``.

    ``t`` holds the P sampling times, finite and non-decreasing (equal
    neighbours are legal; nothing is sorted here, because the model's columns
    follow ``t``); ``data`` the P finite measurements; ``sigma`` the P fixed
    error bars, finite and >= 0 (``None`` = all zero).  ``model`` takes the
    (n, n_dim) batch of points as a torch tensor and returns a pair of
    float64 tensors on the same device: ``m`` the (n, P) mean prediction and
    ``h`` the (n, 3) hyper-parameters with columns (a, l, s) -- signal
    variance, length scale and a jitter variance added in quadrature -- or,
    for 'sho', (n, 4) with a fourth column q.  ``kernel`` is, as a function
    of r = |dt| / l,

      'exp'       exp(-r)                                       1 state
      'matern32'  (1 + sqrt(3) r) exp(-sqrt(3) r)               2 states
      'matern52'  (1 + sqrt(5) r + 5 r^2 / 3) exp(-sqrt(5) r)   3 states
      'sho'       exp(-r / (2 q)) [cos(eta r) + sin(eta r) / (2 eta q)],
                  eta = sqrt(1 - 1 / (4 q^2)), q > 1/2          2 states

    the first three those of ``gp_correlation``, the last the underdamped
    oscillator of frequency 1 / l and quality factor q (``sho_correlation``;
    its critically damped limit q = 1/2 is 'matern32' with l / sqrt(3)).
    The squared exponential has no finite state and is refused.

    A call evaluates the model and then runs the fused kernel
    ``nb_gps_loglike`` -- one launch on the current stream with one lane per
    point, which walks the series once with a state of at most 3 x 3 numbers
    and builds no matrix.  ``from_model`` is the second half alone; it reads
    a cuda tensor whose rows are strided (``stride(1) == 1``, ``stride(0)`` at
    least the width, such as a column slice of a wider tensor) in place and
    copies anything else to contiguous, separately for ``m`` and ``h``.
    ``numpy`` / ``numpy_from_model`` are the pure-numpy twins: the same
    recursion with the same operations in the same order, vectorised over
    the rows.

    A gap enters as min(dt / l, 1e4), the cap of ``gp_correlation``: beyond
    it the two sides are independent (for 'sho' that is so up to q of about
    7; a larger q with a gap beyond 1e4 l sees the gap shortened).

    Row i is NaN when any m_ij is not finite; when a is negative or not
    finite (a = 0 is legal: white noise only), l is outside (0, +inf), s is
    negative or not finite or, for 'sho', q is outside (1/2, +inf); or when a
    pivot of the recursion -- the predictive variance of a measurement given
    the earlier ones -- is outside (0, +inf).  That changes no bit of any
    other row.

    A sum of terms: ``kernel`` may be a tuple or list of 2 or 3 of the names
    above whose states add up to at most 6 (10 pairs and 13 triples up to
    order), such as ``('sho', 'sho')`` for stellar rotation at P and P / 2
    or ``('matern32', 'sho')`` for red noise plus a quasi-periodic term:

        K_jk = sum_i a_i rho_i(|t_j - t_k| / l_i) + delta_jk (sigma_j^2 + s).

    ``h`` is then (n, W) and holds, for every term in the order given,
    (a_i, l_i) or for 'sho' (a_i, l_i, q_i), and s in one last column: W =
    sum w_i + 1 <= 10.  The sum is itself a state-space kernel -- the states
    concatenated, the transition block diagonal -- and the same kind of
    filter walks it with a state of at most 6 x 6 numbers (nb_gps_filter.h,
    whose header states the recursion).  Inside, the terms are sorted by
    kernel, equal names in their order: naming them in another order together
    with their columns changes no bit.  The NaN rules hold for every a_i (a_i
    = 0 is legal and switches the term off), l_i and q_i.  A string keeps the
    single-term path bit for bit; a sequence of one name is refused.  One
    difference from a single term: a repeated time with sigma_j^2 + s = 0,
    which one term answers with a NaN row, is unspecified for a sum -- the
    row is NaN or finite, and no other row is touched."""

    _second = 'hyper-parameters'

    def __init__(self, model, t, data, sigma=None, *, kernel='matern32',
                 normalised=True):
        super().__init__(model)
        terms = (kernel,) if isinstance(kernel, str) or \
            not isinstance(kernel, (tuple, list)) else tuple(kernel)
        for name in terms:
            if isinstance(name, str) and name == 'sqexp':
                raise ValueError("kernel 'sqexp' has no finite state: no "
                                 'filter evaluates it; '
                                 'GaussianProcessLikelihood does, up to %d '
                                 'data points' % N_GP_MAX)
            if not isinstance(name, str) or name not in GPS_KERNELS:
                raise ValueError('kernel must be one of %s, not %r' %
                                 (', '.join(map(repr, GPS_KERNELS)), name))
        if isinstance(kernel, (tuple, list)):
            if len(terms) == 1:
                raise ValueError('a sequence of one kernel name is not a sum: '
                                 'write kernel=%r, the string, for one term' %
                                 terms[0])
            states = sum(GPS_STATES[name] for name in terms)
            if not 2 <= len(terms) <= GPS_MAX_TERMS or \
                    states > GPS_MAX_STATES:
                raise ValueError(
                    'a sum of kernels has at most %d terms and at most %d '
                    'states (exp 1, matern32 2, matern52 3, sho 2), not %d '
                    'terms with %d states' % (GPS_MAX_TERMS, GPS_MAX_STATES,
                                              len(terms), states))
            kernel = terms
            # the slots of nb_gps_filter.h: the terms sorted by kernel code,
            # equal names in their order, each with the column of its a
            first = np.cumsum([0] + [3 if name == 'sho' else 2
                                     for name in terms])
            order = sorted(range(len(terms)),
                           key=lambda i: GPS_KERNELS.index(terms[i]))
            self._slots = tuple((terms[i], int(first[i])) for i in order)
        self.kernel = kernel
        p = self._set_data(data, N_GPS_MAX)
        t = np.asarray(t, float)
        if t.shape != (p,):
            raise ValueError('t must have shape (%d,), not %s' % (p, t.shape))
        if not np.all(np.isfinite(t)):
            raise ValueError('t must be finite')
        with np.errstate(over='ignore'):
            dt = np.diff(t, prepend=t[0])
        if np.any(dt < 0):
            raise ValueError('t must not decrease (it is not sorted here: the '
                             "model's columns follow t)")
        if not np.all(np.isfinite(dt)):
            raise ValueError('t is too spread out: a step is not finite')
        self.t = t.copy()
        self._dt = dt
        self._set_sigma(sigma, normalised)

    @property
    def _width(self):
        return device.gps_width(self.kernel)

    def _make_table(self):
        return device.GPSTable(self.t, self.data, self._sigma2,
                               kernel=self.kernel, log_norm=self.log_norm)

    def from_model(self, m, h):
        """log L of the rows of an (n, P) float64 model output and its (n, 3)
        or (n, 4) hyper-parameters ((n, W) for a sum of terms): cuda tensors
        in, a cuda tensor out; numpy in, numpy out."""
        self._same_kind(m, h)
        return self._from_outputs(m, h)

    @staticmethod
    def _transition(kernel, r, w, eta, inv_eta):
        """Phi of ``kernel`` at the capped r = dt / l of every row, as
        ``gps_phi`` of nb_gps_filter.h builds it: a list of rows of (n,)
        arrays."""
        ty = r.dtype.type
        if kernel == 'exp':
            return [[np.exp(-r)]]
        if kernel == 'matern32':
            x = np.sqrt(ty(3)) * r
            e = np.exp(-x)
            ex = e * x
            return [[e * (1 + x), ex], [-ex, e * (1 - x)]]
        if kernel == 'matern52':
            x = np.sqrt(ty(5)) * r
            e = np.exp(-x)
            x2 = x * x
            hx = ty(0.5) * x2
            return [[e * ((1 + x) + hx), e * (x + x2), e * hx],
                    [-(e * hx), e * ((1 + x) - x2), e * (x - hx)],
                    [e * (hx - x), e * (x2 - 3 * x),
                     e * ((1 - 2 * x) + hx)]]
        e = np.exp(-(r * w))
        arg = eta * r
        c = np.cos(arg)
        sg = np.sin(arg) * inv_eta
        sw = sg * w
        es = e * sg
        return [[e * (c + sw), es], [-es, e * (c - sw)]]

    def numpy_from_model(self, m, h, dtype=np.float64):
        """Pure-numpy evaluation of an (n, P) model output and its
        hyper-parameters (CPU baseline / oracle runs / tests): the recursion
        that nb_gps_filter.h states, with its operations in its order -- the
        slots' blocks of the state one after the other, every sum over slots
        in slot order -- vectorised over the rows, in ``dtype``:
        ``np.longdouble`` gives the tests their truth.  Every ``dtype`` starts
        from the same float64 inputs."""
        m, h = np.asarray(m, float), np.asarray(h, float)
        self._check(m, h)
        ty = np.dtype(dtype).type
        n, p = m.shape
        # (name, column of a, column of q) of every slot, and the column of s
        if isinstance(self.kernel, tuple):
            slots = [(name, col, col + 2) for name, col in self._slots]
            col_s = self._width - 1
        else:
            slots, col_s = [(self.kernel, 0, 3)], 2
        sizes = [GPS_STATES[name] for name, _, _ in slots]
        offs = [sum(sizes[:i]) for i in range(len(slots))]
        rs = range(sum(sizes))
        with np.errstate(all='ignore'):
            s = h[:, col_s].astype(ty)
            bad = ~((s >= 0) & (s < np.inf))
            rows = []                            # a, 1 / l, w, eta, 1 / eta
            for name, col, col_q in slots:
                a, l = h[:, col].astype(ty), h[:, col + 1].astype(ty)
                bad |= ~((a >= 0) & (a < np.inf)) | ~((l > 0) & (l < np.inf))
                inv_l = np.minimum(1 / l, ty(np.finfo(np.float64).max))
                w = eta = inv_eta = None
                if name == 'sho':
                    q = h[:, col_q].astype(ty)
                    bad |= ~((q > 0.5) & (q < np.inf))
                    w = 1 / (2 * q)
                    eta = np.sqrt(1 - w * w)
                    inv_eta = 1 / eta
                rows.append((a, inv_l, w, eta, inv_eta))
            total = sum_in_order(row[0] for row in rows)
            zero = np.zeros(n, ty)
            big_g = [[zero for _ in rs] for _ in rs]
            g = [zero for _ in rs]
            q_sum, q_low, l_sum = zero, zero, zero
            md = m.astype(ty)
            for j in range(p):
                phis = [self._transition(
                    name, np.minimum(ty(self._dt[j]) * inv_l, ty(GPS_CAP)), w,
                    eta, inv_eta)
                    for (name, _, _), (_, inv_l, w, eta, inv_eta)
                    in zip(slots, rows)]
                # 1. the lower blocks, mirrored; then g
                for bi, (oi, ri, phi_i) in enumerate(zip(offs, sizes, phis)):
                    for bj in range(bi + 1):
                        oj, rj, phi_j = offs[bj], sizes[bj], phis[bj]
                        t = [[sum_in_order(phi_i[i][k] * big_g[oi + k][oj + c]
                                           for k in range(ri))
                              for c in range(rj)] for i in range(ri)]
                        for i in range(ri):
                            for c in range(i + 1 if bi == bj else rj):
                                big_g[oi + i][oj + c] = \
                                    big_g[oj + c][oi + i] = sum_in_order(
                                        t[i][k] * phi_j[c][k]
                                        for k in range(rj))
                gn = [None for _ in rs]
                for oi, ri, phi_i in zip(offs, sizes, phis):
                    for i in range(ri):
                        gn[oi + i] = sum_in_order(phi_i[i][k] * g[oi + k]
                                                  for k in range(ri))
                # 2. what the observation sees of G, and the pivot
                gh = [sum_in_order(big_g[i][o] for o in offs) for i in rs]
                c_sum = sum_in_order(gh[o] for o in offs)
                g_sum = sum_in_order(gn[o] for o in offs)
                noise = ty(self._sigma2[j]) + s
                d = (total - c_sum) + noise
                # 3.
                v = (md[:, j] - ty(self.data[j])) - g_sum
                bad |= ~np.isfinite(md[:, j]) | ~((d > 0) & (d < np.inf))
                inv_d = 1 / d
                # 4. u = a p - Gh, p = [1], [1, 0], [1, 0, -1/3], [1, 0]
                u = [None for _ in rs]
                for o, r, row in zip(offs, sizes, rows):
                    u[o] = row[0] - gh[o]
                    if r > 1:
                        u[o + 1] = -gh[o + 1]
                    if r > 2:
                        u[o + 2] = row[0] * -(1 / ty(3)) - gh[o + 2]
                k = [u[i] * inv_d for i in rs]
                # 5.
                g = [gn[i] + k[i] * v for i in rs]
                for i in rs:
                    for c in range(i + 1):
                        big_g[i][c] = big_g[c][i] = big_g[i][c] + u[i] * k[c]
                if len(slots) == 1:
                    # G00 + u0 k0 in the form that is a exactly without noise
                    big_g[0][0] = rows[0][0] - noise * k[0]
                # 6.
                y = (v * v) * inv_d - q_low          # a compensated sum
                q_new = q_sum + y
                q_low = (q_new - q_sum) - y
                q_sum = q_new
                l_sum = l_sum + np.log(d)
            out = ty(self.log_norm) - ty(0.5) * (q_sum + l_sum)
        return np.where(bad, ty(np.nan), out)


class RosenbrockLikelihood:
    """Rosenbrock function on x = low + (high - low) u (BASELINE config 3):
    log L = -sum_i [a (x_{i+1} - x_i^2)^2 + (1 - x_i)^2] --
    ``nb_loglike_rosenbrock``."""

    device = True

    def __init__(self, n_dim, low=-5.0, high=5.0, a=100.0):
        self.n_dim = int(n_dim)
        self.low, self.high, self.a = float(low), float(high), float(a)

    def __call__(self, x):
        from . import _lib
        lib = _lib.load()
        xs = device.as_device_points(x, self.n_dim)
        out = torch.empty(xs.shape[0], dtype=torch.float64, device='cuda')
        _lib.check(lib.nb_loglike_rosenbrock(
            device._ptr(xs), xs.shape[0], self.n_dim, self.low, self.high,
            self.a, device._ptr(out), device._stream()))
        return out if isinstance(x, torch.Tensor) else out.cpu().numpy()

    def numpy(self, x):
        """Pure-numpy evaluation (CPU baseline / oracle runs / tests)."""
        x = self.low + (self.high - self.low) * np.atleast_2d(x)
        return -np.sum(self.a * (x[:, 1:] - x[:, :-1]**2)**2 +
                       (1.0 - x[:, :-1])**2, axis=1)


class FunnelLikelihood:
    """Neal's funnel in n_dim dimensions on the unit cube (BASELINE config 5;
    the reference's tests/test_sampler.py:311-314 has the 2-D case):
    x_0 ~ N(mu, sigma0^2), x_i ~ N(mu, (exp(k (x_0 - mu)) / c)^2) for i > 0 --
    ``nb_loglike_funnel``."""

    device = True

    def __init__(self, n_dim, mu=0.5, sigma0=0.1, k=20.0, c=100.0):
        self.n_dim = int(n_dim)
        self.mu, self.sigma0 = float(mu), float(sigma0)
        self.k, self.c = float(k), float(c)

    def __call__(self, x):
        from . import _lib
        lib = _lib.load()
        xs = device.as_device_points(x, self.n_dim)
        out = torch.empty(xs.shape[0], dtype=torch.float64, device='cuda')
        _lib.check(lib.nb_loglike_funnel(
            device._ptr(xs), xs.shape[0], self.n_dim, self.mu, self.sigma0,
            self.k, self.c, device._ptr(out), device._stream()))
        return out if isinstance(x, torch.Tensor) else out.cpu().numpy()

    def numpy(self, x):
        from scipy.stats import norm
        x = np.atleast_2d(x)
        s = np.exp(self.k * (x[:, 0] - self.mu)) / self.c
        return (norm.logpdf(x[:, 0], loc=self.mu, scale=self.sigma0) +
                np.sum(norm.logpdf(x[:, 1:], loc=self.mu,
                                   scale=s[:, None]), axis=1))
