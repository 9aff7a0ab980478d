"""Host side of the device prior transform: which priors get a device table
(``Prior.device_table``), what it holds, and how long it is cached.  No GPU
needed."""

import pickle

import numpy as np
from scipy import stats

from nautilus_amd import Prior


def _mixed_prior():
    """One parameter of each kind, arguments given positionally and by
    keyword, a fixed and two tied keys in between."""
    p = Prior()
    p.add_parameter('flat', dist=(-3, 5))
    p.add_parameter('gauss', dist=stats.norm(loc=2.0, scale=0.5))
    p.add_parameter('fixed', dist=1.5)
    p.add_parameter('amp', dist=stats.loguniform(1e-3, 10.0))
    p.add_parameter('amp2', dist=stats.reciprocal(a=1.0, b=2.0, scale=3.0))
    p.add_parameter('tied', dist='amp')
    p.add_parameter('width', dist=stats.lognorm(0.7, 1.0, 2.0))
    p.add_parameter('width2', dist=stats.lognorm(s=2.5, scale=4.0))
    p.add_parameter('pos', dist=stats.halfnorm(scale=3.0))
    p.add_parameter('tied_fixed', dist='fixed')
    p.add_parameter('cut', dist=stats.truncnorm(-1.0, 2.0, loc=0.5, scale=2.0))
    p.add_parameter('cut2', dist=stats.truncnorm(a=5.0, b=np.inf))
    return p


def test_device_table_of_every_kind():
    p = _mixed_prior()
    t = p.device_table()
    assert p.device and t is not None
    assert t.kind.dtype == np.uint8 and t.key_column.dtype == np.int32
    assert t.kind.tolist() == [0, 1, 2, 2, 3, 3, 4, 5, 5]
    assert t.loc.tolist() == [-3, 2.0, 0, 0, 1.0, 0, 0, 0.5, 0]
    assert t.scale.tolist() == [8, 0.5, 1, 3.0, 2.0, 4.0, 3.0, 2.0, 1]
    assert t.shape0.tolist() == [0, 0, 1e-3, 1.0, 0.7, 2.5, 0, -1.0, 5.0]
    assert t.shape1.tolist() == [0, 0, 10.0, 2.0, 0, 0, 0, 2.0, np.inf]
    # keys in order: own column, -1 with the constant, or the root's entry
    assert t.key_column.tolist() == [0, 1, -1, 2, 3, 2, 4, 5, 6, -1, 7, 8]
    assert t.key_value.tolist() == [0, 0, 1.5, 0, 0, 0, 0, 0, 0, 1.5, 0, 0]
    assert len(t.key_column) == len(p.keys)


def test_other_families_stay_on_the_host():
    for dist in (stats.beta(2.0, 3.0), stats.expon(),
                 stats.truncnorm(1e200, np.inf), stats.loguniform(1.0, np.inf)):
        p = _mixed_prior()
        assert p.device
        p.add_parameter('other', dist=dist)
        assert p.device_table() is None and not p.device
        assert p.device_spec() is None
        # the host path does not care
        assert p.unit_to_physical(np.full((2, 10), 0.5)).shape == (2, 10)


def test_table_is_cached_until_the_prior_changes():
    p = _mixed_prior()
    t = p.device_table()
    assert p.device_table() is t
    p.add_parameter('late', dist=(0, 1))
    t2 = p.device_table()
    assert t2 is not t and len(t2.kind) == len(t.kind) + 1
    # keys and dists are public lists: an edit in place is seen as well
    p.dists[0] = stats.norm(loc=1.0, scale=2.0)
    t3 = p.device_table()
    assert t3 is not t2 and t3.kind[0] == 1 and t3.loc[0] == 1.0
    p.dists[0] = stats.beta(2.0, 3.0)
    assert p.device_table() is None and not p.device
    p.dists[0] = stats.uniform(loc=-3, scale=8)
    p.keys[0] = 'renamed'
    assert p.device_table() is not t3 and p.device_table().kind[0] == 0


def test_pickled_prior_gives_the_same_table():
    p = _mixed_prior()
    t = p.device_table()
    q = pickle.loads(pickle.dumps(p))
    assert '_device_cache' not in q.__dict__
    t2 = q.device_table()
    for a, b in zip(t, t2):
        assert a.dtype == b.dtype and np.array_equal(a, b)
    assert q.keys == p.keys


def test_device_spec_is_unchanged():
    p = Prior()
    p.add_parameter('a', dist=(-3, 5))
    p.add_parameter('b', dist=stats.norm(loc=2.0, scale=0.5))
    p.add_parameter('c', dist=1.5)
    p.add_parameter('d', dist='a')
    kind, loc, scale = p.device_spec()
    assert kind.tolist() == [0, 1]
    assert loc.tolist() == [-3, 2.0] and scale.tolist() == [8, 0.5]
    # a family that only the table covers: no (kind, loc, scale) triple
    p.add_parameter('e', dist=stats.loguniform(1.0, 2.0))
    assert p.device_spec() is None and p.device


def test_error_names_the_parameter_and_the_families():
    import pytest
    import torch
    p = _mixed_prior()
    p.add_parameter('shape', dist=stats.beta(2.0, 3.0))
    p.add_parameter('rate', dist=stats.expon())
    with pytest.raises(ValueError) as err:
        p.unit_to_physical(torch.zeros(2, 11, dtype=torch.float64))
    assert "'shape'" in str(err.value) and 'truncnorm' in str(err.value)
    assert "'rate'" not in str(err.value)

    def like(x):
        return x['flat']
    like.device = True
    from nautilus_amd import Sampler
    with pytest.raises(ValueError) as err:
        Sampler(p, like)
    assert "'shape'" in str(err.value) and 'loguniform' in str(err.value)
