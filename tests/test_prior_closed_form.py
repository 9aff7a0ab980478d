"""Host side of the closed-form tier of the device prior transform (kinds 7
to 17: cauchy, halfcauchy, laplace, logistic, gumbel_r, gumbel_l,
weibull_min, rayleigh, pareto, powerlaw, triang): which priors get a device
table, what it holds, which shapes keep a prior on the host -- and that scipy
itself lies inside the band in which the GPU tests compare with the exact
quantiles of ``tests/golden/quantile_exact.npz``.  No GPU needed."""

import pickle

import numpy as np
import pytest
from scipy import stats

from conftest import load_golden
from nautilus_amd import Prior
from nautilus_amd.prior import DEVICE_FAMILIES, DEVICE_KINDS

NAMES = ['cauchy', 'halfcauchy', 'laplace', 'logistic', 'gumbel_r',
         'gumbel_l', 'weibull_min', 'rayleigh', 'pareto', 'powerlaw',
         'triang']


def _closed_form_prior():
    """One parameter of each new family with loc / scale, shapes given
    positionally and by keyword, a fixed and a tied key in between."""
    p = Prior()
    p.add_parameter('k7', dist=stats.cauchy(loc=1.0, scale=2.0))
    p.add_parameter('k8', dist=stats.halfcauchy(0.5, 3.0))
    p.add_parameter('fixed', dist=1.5)
    p.add_parameter('k9', dist=stats.laplace(loc=-1.0, scale=0.25))
    p.add_parameter('k10', dist=stats.logistic(2.0, scale=0.5))
    p.add_parameter('k11', dist=stats.gumbel_r(loc=0.5, scale=1.5))
    p.add_parameter('tied', dist='k9')
    p.add_parameter('k12', dist=stats.gumbel_l(scale=4.0))
    p.add_parameter('k13', dist=stats.weibull_min(2.5, 1.0, 2.0))
    p.add_parameter('k13b', dist=stats.weibull_min(c=0.3, scale=5.0))
    p.add_parameter('k14', dist=stats.rayleigh(loc=0.125, scale=0.75))
    p.add_parameter('k15', dist=stats.pareto(3.0, loc=-2.0, scale=2.0))
    p.add_parameter('k15b', dist=stats.pareto(b=0.5))
    p.add_parameter('k16', dist=stats.powerlaw(3.5, 1.0, 4.0))
    p.add_parameter('k16b', dist=stats.powerlaw(a=0.2, loc=0.5))
    p.add_parameter('k17', dist=stats.triang(0.3, loc=-1.0, scale=2.0))
    p.add_parameter('k17b', dist=stats.triang(c=1.0, scale=8.0))
    p.add_parameter('k17c', dist=stats.triang(c=0.0))
    return p


def test_kinds_and_names():
    assert [DEVICE_KINDS[n][0] for n in NAMES] == list(range(7, 18))
    assert [DEVICE_KINDS[n][1] for n in NAMES] == \
        [0, 0, 0, 0, 0, 0, 1, 0, 1, 1, 1]
    assert 6 not in [k for k, _ in DEVICE_KINDS.values()]
    for name in NAMES + ['truncnorm', 'loguniform']:
        assert name in DEVICE_FAMILIES


def test_device_table_of_every_new_kind():
    p = _closed_form_prior()
    t = p.device_table()
    assert p.device and t is not None
    assert t.kind.dtype == np.uint8
    assert t.kind.tolist() == [7, 8, 9, 10, 11, 12, 13, 13, 14, 15, 15, 16,
                               16, 17, 17, 17]
    assert t.loc.tolist() == [1.0, 0.5, -1.0, 2.0, 0.5, 0, 1.0, 0, 0.125,
                              -2.0, 0, 1.0, 0.5, -1.0, 0, 0]
    assert t.scale.tolist() == [2.0, 3.0, 0.25, 0.5, 1.5, 4.0, 2.0, 5.0, 0.75,
                                2.0, 1, 4.0, 1, 2.0, 8.0, 1]
    assert t.shape0.tolist() == [0, 0, 0, 0, 0, 0, 2.5, 0.3, 0, 3.0, 0.5,
                                 3.5, 0.2, 0.3, 1.0, 0.0]
    assert not t.shape1.any()
    assert t.key_column.tolist() == [0, 1, -1, 2, 3, 4, 2, 5, 6, 7, 8, 9, 10,
                                     11, 12, 13, 14, 15]
    assert t.key_value[2] == 1.5
    # the host path is scipy's
    u = np.random.default_rng(1).random((4, 16))
    x = p.unit_to_physical(u)
    assert np.array_equal(x[:, 9], stats.pareto(3.0, -2.0, 2.0).isf(1 - u[:, 9]))


def test_new_and_old_kinds_mix():
    p = _closed_form_prior()
    p.add_parameter('flat', dist=(-3, 5))
    p.add_parameter('cut', dist=stats.truncnorm(5.0, np.inf))
    t = p.device_table()
    assert t.kind.tolist()[-2:] == [0, 5] and t.shape1[-1] == np.inf


@pytest.mark.parametrize('dist,word', [
    (stats.weibull_min(0), 'weibull_min'), (stats.weibull_min(-2.0), 'c > 0'),
    (stats.pareto(-1), 'pareto'), (stats.pareto(np.inf), 'b > 0'),
    (stats.pareto(1e-320), 'pareto'),
    (stats.powerlaw(0.0), 'powerlaw'), (stats.powerlaw(np.inf), 'a > 0'),
    (stats.powerlaw(np.nan), 'powerlaw'),
    (stats.triang(1.5), 'triang'), (stats.triang(-0.1), '0 <= c <= 1'),
    (stats.triang(np.nan), 'triang'), (stats.weibull_min(np.inf), 'finite'),
    (stats.cauchy(scale=0.0), 'scale'), (stats.laplace(loc=np.inf), 'loc')])
def test_invalid_shapes_stay_on_the_host(dist, word):
    p = _closed_form_prior()
    p.add_parameter('bad one', dist=dist)
    assert p.device_table() is None and not p.device
    reason = p._cached()['obstacle']
    assert reason.startswith("parameter 'bad one': ") and word in reason
    import torch
    with pytest.raises(ValueError) as err:
        p.unit_to_physical(torch.zeros(2, 17, dtype=torch.float64))
    assert "'bad one'" in str(err.value) and word in str(err.value)
    assert 'truncnorm' in str(err.value) and 'halfcauchy' in str(err.value)


def test_expon_and_beta_still_stay_on_the_host():
    for dist in (stats.expon(), stats.expon(scale=2.0), stats.beta(2.0, 3.0)):
        p = _closed_form_prior()
        p.add_parameter('other', dist=dist)
        assert p.device_table() is None and not p.device
    # ... and the device spelling of an exponential prior is the same law
    u = np.linspace(0.01, 0.99, 50)
    assert np.allclose(stats.weibull_min(1, loc=0.5, scale=2.0).isf(u),
                       stats.expon(loc=0.5, scale=2.0).isf(u), rtol=1e-15)
    p = Prior()
    p.add_parameter('rate', dist=stats.weibull_min(1, loc=0.5, scale=2.0))
    assert p.device and p.device_table().kind.tolist() == [13]


def test_pickled_prior_gives_the_same_table():
    p = _closed_form_prior()
    t = p.device_table()
    assert '_device_cache' in p.__dict__
    q = pickle.loads(pickle.dumps(p))
    assert '_device_cache' not in q.__dict__
    t2 = q.device_table()
    for a, b in zip(t, t2):
        assert a.dtype == b.dtype and np.array_equal(a, b)
    assert q.keys == p.keys and q.device


# ---- the fixture -------------------------------------------------------------

def test_fixture_holds_what_the_gpu_tests_need():
    g = load_golden('quantile_exact')
    u = g['u']
    assert u.shape == (1005,) and np.all(np.diff(u) > 0)
    assert u[0] == 1e-6 and u[-1] == 1 - 1e-6
    for v in (0.25, 0.5, 0.75, np.exp(-1.0), 1 - np.exp(-1.0)):
        assert v in u
    # dense towards both ends: as many points below 1e-3 as above 1 - 1e-3,
    # and each of these thousandths holds more than a fifth of all
    assert np.sum(u < 1e-3) == np.sum(u > 1 - 1e-3) > 200
    names = [str(n) for n in g['names']]
    want = {'weibull_min': [0.3, 1, 2.5, 8], 'pareto': [0.5, 1, 3, 20],
            'powerlaw': [0.2, 1, 3.5], 'triang': [0, 0.3, 0.5, 1]}
    cases = [(n, s) for n in NAMES for s in want.get(n, [np.nan])]
    assert len(names) == len(cases) == 22
    for k, (n, s) in enumerate(cases):
        assert names[k] == n
        assert g['shapes'][k] == s or (np.isnan(s) and np.isnan(g['shapes'][k]))
    assert g['exact'].shape == (22, 1005) and np.all(np.isfinite(g['exact']))
    assert g['scipy_dev'].shape == (22,)


def test_scipy_is_inside_the_band_on_the_fixture():
    """|scipy - exact| <= 1e-13 + 1e-12 |exact| for every family and shape,
    recomputed here and equal to what the fixture recorded (in units of the
    band); the largest is far below 1, so the band of the GPU tests is a
    condition with room, not a measurement of this code."""
    g = load_golden('quantile_exact')
    q = 1.0 - g['u']
    worst = {}
    for k, name in enumerate(str(n) for n in g['names']):
        shape = g['shapes'][k]
        dist = getattr(stats, name)(*([] if np.isnan(shape) else [shape]))
        exact = g['exact'][k]
        dev = np.max(np.abs(dist.isf(q) - exact) / (1e-13 + 1e-12 * np.abs(exact)))
        worst[name] = max(worst.get(name, 0.0), dev)
        # the recording, but for the libm of the machine that made it
        assert abs(dev - g["scipy_dev"][k]) <= 0.01, (name, shape)
        assert dev <= 1.0, (name, shape, dev)
    for name, dev in worst.items():
        print('%s: scipy at most %.2e of the band from the exact quantile' %
              (name, dev))
