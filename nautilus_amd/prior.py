"""Prior helper with the interface of ``nautilus.Prior`` (reference
nautilus/prior.py:9-181): named parameters that are free (a distribution
with an ``isf`` method), fixed (a number) or tied to an earlier parameter (its
name).  Numpy points are transformed on the host; cuda tensors (the batches of
a device likelihood) are transformed on the GPU when every free parameter is
a frozen scipy distribution of one of the families in ``DEVICE_KINDS``
(``nb_prior_table_transform``): the uniform,
normal and log families, and the families whose quantile function is a closed
form -- ``cauchy``, ``halfcauchy``, ``laplace``, ``logistic``, ``gumbel_r``,
``gumbel_l``, ``weibull_min``, ``rayleigh``, ``pareto``, ``powerlaw`` and
``triang``."""

import collections
import numbers

import numpy as np
from scipy.stats import uniform

FREE, FIXED, TIED = 'free', 'fixed', 'tied'

# scipy name -> (kind of the device table, number of shape parameters)
DEVICE_KINDS = {'uniform': (0, 0), 'norm': (1, 0), 'loguniform': (2, 2),
                'reciprocal': (2, 2), 'lognorm': (3, 1), 'halfnorm': (4, 0),
                'truncnorm': (5, 2),
                # kind 6 is the device's own (a truncnorm in log space)
                'cauchy': (7, 0), 'halfcauchy': (8, 0), 'laplace': (9, 0),
                'logistic': (10, 0), 'gumbel_r': (11, 0), 'gumbel_l': (12, 0),
                'weibull_min': (13, 1), 'rayleigh': (14, 0),
                'pareto': (15, 1), 'powerlaw': (16, 1), 'triang': (17, 1)}
DEVICE_FAMILIES = ('uniform, norm, loguniform (reciprocal), lognorm, '
                   'halfnorm, truncnorm, cauchy, halfcauchy, laplace, '
                   'logistic, gumbel_r, gumbel_l, weibull_min, rayleigh, '
                   'pareto, powerlaw, triang')
# kind -> (scipy's name of the family, of its shape), shape > 0 required
POSITIVE_SHAPE = {13: ('weibull_min', 'c'), 15: ('pareto', 'b'),
                  16: ('powerlaw', 'a')}
# NB_PRIOR_TRUNCNORM_MAX: the device refuses a truncnorm further out
TRUNCNORM_MAX = 1e150

DeviceTable = collections.namedtuple(
    'DeviceTable',
    'kind loc scale shape0 shape1 key_column key_value')


def _device_row(dist):
    """(kind, loc, scale, shape0, shape1) of a free parameter that the device
    can transform, or the reason (a string) why it cannot."""
    name = getattr(getattr(dist, 'dist', None), 'name', None)
    if name not in DEVICE_KINDS:
        return 'its distribution is not a frozen scipy distribution of ' \
            'these families'
    kind, n_shapes = DEVICE_KINDS[name]
    try:
        shapes, loc, scale = dist.dist._parse_args(*dist.args, **dist.kwds)
        row = [float(v) for v in (loc, scale) + tuple(shapes)]
    except Exception:
        return 'its arguments are not plain numbers'
    if len(row) != 2 + n_shapes:
        return 'its arguments are not plain numbers'
    row += [0.0] * (4 - len(row))
    loc, scale, s0, s1 = row
    if not (np.isfinite(loc) and np.isfinite(scale) and scale > 0):
        return 'its loc is not finite or its scale not positive'
    if kind == 2 and not 0 < s0 < s1 < np.inf:
        return 'loguniform needs 0 < a < b'
    if kind == 3 and not 0 < s0 < np.inf:
        return 'lognorm needs s > 0'
    if kind == 5 and not s0 < s1:
        return 'truncnorm needs a < b'
    if kind == 5 and (s0 > TRUNCNORM_MAX or s1 < -TRUNCNORM_MAX):
        return 'its interval lies more than %g standard deviations from ' \
            'the mean' % TRUNCNORM_MAX
    if kind in POSITIVE_SHAPE and not (0 < s0 < np.inf and
                                       np.isfinite(1.0 / s0)):
        return '%s needs a finite %s > 0' % POSITIVE_SHAPE[kind]
    if kind == 17 and not 0 <= s0 <= 1:
        return 'triang needs 0 <= c <= 1'
    return (kind, loc, scale, s0, s1)


def _kind(dist):
    if hasattr(dist, 'isf'):
        return FREE
    if isinstance(dist, numbers.Number):
        return FIXED
    if isinstance(dist, str):
        return TIED
    return None


class Prior:
    """Ordered table of model parameters.  ``keys`` and ``dists`` are the
    reference's public attributes (prior.py:22-23); everything else is derived
    from them through ``_table``."""

    def __init__(self):
        self.keys = []
        self.dists = []

    def add_parameter(self, key=None, dist=(0, 1)):
        """prior.py:25-73: ``dist`` is a (low, high) tuple (uniform), an
        object with ``isf``, a number (fixed) or the name of an earlier
        parameter (tied; chains of names resolve to their root)."""
        if key is not None and not isinstance(key, str):
            raise TypeError("Keyword argument 'key' must be a string.")
        if key is not None and key in self.keys:
            raise ValueError("Key '{}' already in key list.".format(key))
        if isinstance(dist, tuple):
            dist = uniform(loc=dist[0], scale=dist[1] - dist[0])
        kind = _kind(dist)
        if kind is None:
            raise TypeError("Keyword argument 'dist' does not have the "
                            "correct type")
        if kind == TIED:
            if dist not in self.keys or dist == str(key):
                raise ValueError('Key {} not defined previously.'.format(dist))
            while _kind(self.dists[self.keys.index(dist)]) == TIED:
                dist = self.dists[self.keys.index(dist)]
        self.keys.append('x_{}'.format(len(self.keys)) if key is None else key)
        self.dists.append(dist)

    def _table(self):
        """[(key, kind, dist, column of the free parameter or None)]."""
        rows, column = [], 0
        for key, dist in zip(self.keys, self.dists):
            kind = _kind(dist)
            rows.append((key, kind, dist, column if kind == FREE else None))
            column += kind == FREE
        return rows

    def dimensionality(self):
        return sum(kind == FREE for _, kind, _, _ in self._table())

    def _require_width(self, width):
        if self.dimensionality() != width:
            raise ValueError('Dimensionality of points does not match prior.')

    def device_spec(self):
        """(kind, loc, scale) arrays if every free parameter is a frozen scipy
        ``uniform`` (kind 0) or ``norm`` (kind 1), else None -- the arguments
        of ``nb_prior_transform``.  ``device_table`` covers more families."""
        kind, loc, scale = [], [], []
        for _, row_kind, dist, _ in self._table():
            if row_kind != FREE:
                continue
            name = getattr(getattr(dist, 'dist', None), 'name', None)
            if name not in ('uniform', 'norm'):
                return None
            try:
                _, lo, sc = dist.dist._parse_args(*dist.args, **dist.kwds)
            except Exception:
                return None
            kind.append(0 if name == 'uniform' else 1)
            loc.append(float(lo))
            scale.append(float(sc))
        return np.array(kind, np.uint8), np.array(loc), np.array(scale)

    def _cached(self):
        """The cache of everything derived for the device, emptied when
        ``keys`` or ``dists`` no longer hold the objects it was built from
        (both are public lists that may be edited in place; the cache keeps
        the objects alive, so identity is a safe test)."""
        cache = self.__dict__.get('_device_cache')
        if cache is not None and cache['keys'] == self.keys and \
                len(cache['dists']) == len(self.dists) and \
                all(a is b for a, b in zip(cache['dists'], self.dists)):
            return cache
        cache = dict(keys=list(self.keys), dists=list(self.dists), handles={})
        cache['table'], cache['obstacle'] = self._build_device_table()
        self._device_cache = cache
        return cache

    def _build_device_table(self):
        """(DeviceTable, None), or (None, why the first parameter that the
        device cannot transform keeps the prior on the host)."""
        rows, key_column, key_value = [], [], []
        for key, row_kind, dist, column in self._table():
            if row_kind == FREE:
                row = _device_row(dist)
                if isinstance(row, str):
                    return None, "parameter '%s': %s" % (key, row)
                rows.append(row)
                key_column.append(column)
                key_value.append(0.0)
            elif row_kind == FIXED:
                key_column.append(-1)
                key_value.append(float(dist))
            else:
                # a tied key shows its root (add_parameter resolves chains);
                # the root may itself be fixed
                root = self.keys.index(dist) if dist in self.keys else -1
                if not 0 <= root < len(key_column):
                    return None, "parameter '%s': tied to '%s', which is " \
                        "not an earlier parameter" % (key, dist)
                key_column.append(key_column[root])
                key_value.append(key_value[root])
        if not rows:
            return None, 'the prior has no free parameter'
        if len(rows) > 128:
            return None, 'more than 128 free parameters'
        cols = list(zip(*rows))
        return DeviceTable(
            np.array(cols[0], np.uint8), np.array(cols[1]), np.array(cols[2]),
            np.array(cols[3]), np.array(cols[4]),
            np.array(key_column, np.int32), np.array(key_value)), None

    def device_table(self):
        """The table that ``nb_prior_table_create`` takes -- per free
        parameter ``kind`` (``DEVICE_KINDS``), scipy's ``loc`` / ``scale`` and
        up to two shapes (given positionally or by keyword); per key of the
        prior ``key_column`` (its column, its root's column, or -1 for a fixed
        value) and ``key_value`` -- or None if a free parameter is of another
        family.  Cached until ``keys`` / ``dists`` change.

        ``expon`` is deliberately not a device kind, simple as its transform
        is: ``tests/test_host_logic.py::test_prior_device_spec`` uses it as
        the example of a distribution that keeps a prior on the host.
        ``weibull_min(1, loc=..., scale=...)`` is the device spelling of an
        exponential prior.  The closed-form families (kinds 7 to 17) take no
        shape, except ``weibull_min`` (c > 0), ``pareto`` (b > 0),
        ``powerlaw`` (a > 0) and ``triang`` (0 <= c <= 1), whose one shape is
        ``shape0``; a shape outside its range keeps the prior on the host,
        as scipy itself would only return nan for it."""
        return self._cached()['table']

    @property
    def device(self):
        """True if batches can be transformed on the GPU."""
        return self.device_table() is not None

    def _device_handle(self):
        """``device.PriorTable`` of the current GPU (uploaded once)."""
        import torch
        from . import device
        cache = self._cached()
        if cache['table'] is None:
            raise ValueError(
                'this prior cannot be transformed on the device (%s); '
                'supported are frozen scipy distributions of the families %s, '
                'fixed and tied parameters' % (cache['obstacle'],
                                               DEVICE_FAMILIES))
        index = torch.cuda.current_device()
        if index not in cache['handles']:
            cache['handles'][index] = device.PriorTable(*cache['table'])
        return cache['handles'][index]

    def __getstate__(self):
        # device handles stay behind (a Prior travels to pool workers)
        state = dict(self.__dict__)
        state.pop('_device_cache', None)
        return state

    def unit_to_physical(self, points):
        """x = dist.isf(1 - u) for every free parameter (prior.py:85-120);
        a cuda tensor is transformed on the device, a numpy array by scipy."""
        import torch
        if isinstance(points, torch.Tensor):
            handle = self._device_handle()
            self._require_width(points.shape[-1])
            return handle.transform(points)
        points = np.asarray(points)
        self._require_width(points.shape[-1])
        physical = np.zeros_like(points)
        for _, kind, dist, column in self._table():
            if kind == FREE:
                physical[..., column] = dist.isf(1 - points[..., column])
        return physical

    def physical_to_dictionary(self, phys_points):
        """One entry per key: the column of a free parameter, a constant array
        for a fixed one, the entry of its root for a tied one
        (prior.py:122-162; numpy arrays or cuda tensors)."""
        import torch
        if isinstance(phys_points, torch.Tensor):
            constant = torch.full_like
        else:
            phys_points = np.asarray(phys_points)
            self._require_width(phys_points.shape[-1])
            constant = np.full_like
        table = self._table()
        values = {}
        for key, kind, dist, column in table:
            if kind == FREE:
                values[key] = phys_points[..., column]
            elif kind == FIXED:
                values[key] = constant(phys_points[..., 0], dist)
        for key, kind, dist, _ in table:
            if kind == TIED:
                values[key] = values[dist]
        return {key: values[key] for key in self.keys}

    def unit_to_dictionary(self, points):
        """prior.py:164-181.  For a cuda tensor every value is a contiguous
        row of one (number of keys, n) tensor that the device kernel writes
        directly: fixed parameters filled in, tied ones written a second
        time."""
        import torch
        if isinstance(points, torch.Tensor):
            from . import device
            handle = self._device_handle()
            self._require_width(points.shape[-1])
            rows = handle.transform(points, device.COLUMN_MAJOR)
            return {key: rows[k] for k, key in enumerate(self.keys)}
        return self.physical_to_dictionary(self.unit_to_physical(points))
