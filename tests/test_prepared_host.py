"""CPU, no library: ops._prepared, the one place where prepared operands are cached on a module."""
import gc
import weakref

import numpy as np

from eqxvision_amd import nn
from eqxvision_amd.ops import _prepared


class _Payload:
    pass


def _counting():
    n = [0]

    def build():
        n[0] += 1
        return _Payload()
    return n, build


def _bn(c=4):
    bn = nn.BatchNorm(c, axis_name="batch")
    bn.state_index.value = (np.zeros(c, np.float32), np.ones(c, np.float32))
    return bn


def _lin():
    return _bn()                                      # any Module: only its cache is used


def test_same_deps_hit():
    mod, leaf = _lin(), np.ones(3, np.float32)
    n, build = _counting()
    a = _prepared(mod, ("t", 1), (leaf, None), build)
    assert _prepared(mod, ("t", 1), (leaf, None), build) is a and n[0] == 1
    assert _prepared(mod, ("t", 2), (leaf, None), build) is not a and n[0] == 2          # another static variant


def test_batchnorm_version_rebuilds_in_place():
    mod, bn = _lin(), _bn()
    n, build = _counting()
    a = _prepared(mod, "t", (bn,), build)
    bn.state_index.value = (np.ones(4, np.float32), np.ones(4, np.float32))              # bumps the version
    b = _prepared(mod, "t", (bn,), build)
    assert b is not a and n[0] == 2 and _prepared(mod, "t", (bn,), build) is b and n[0] == 2
    assert len(mod._cache()["t"]) == 1                                                   # the stale operands are gone
    ref = weakref.ref(a)
    del a
    gc.collect()
    assert ref() is None


def test_equal_but_distinct_dep_rebuilds():
    mod, leaf = _lin(), np.ones(3, np.float32)
    n, build = _counting()
    a = _prepared(mod, "t", (leaf,), build)
    twin = leaf.copy()
    assert np.array_equal(twin, leaf) and _prepared(mod, "t", (twin,), build) is not a and n[0] == 2


def test_entry_keeps_its_deps_alive():
    mod, dep = _lin(), _bn()
    n, build = _counting()
    a = _prepared(mod, "t", (dep,), build)
    ref = weakref.ref(dep)
    del dep
    gc.collect()
    assert ref() is not None                          # so no new object can take its identity while the entry exists
    assert _prepared(mod, "t", (ref(),), build) is a and n[0] == 1


def test_two_dep_sets_under_one_tag():
    mod, x, y = _lin(), _bn(), _bn()
    n, build = _counting()
    a, b = _prepared(mod, "t", (x,), build), _prepared(mod, "t", (y,), build)
    for _ in range(3):
        assert _prepared(mod, "t", (x,), build) is a and _prepared(mod, "t", (y,), build) is b
    assert n[0] == 2
