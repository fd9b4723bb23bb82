"""The receding-horizon fixtures tests/golden/receding_*.npz (recorded from the reference build by
tests/golden/make_receding_goldens.py): the CPU restatement reproduces the whole chain — cold solve, shift by s steps with
the last control held, initial roll-out from the plan's own x[s], warm solve — exactly; so does the reference build where
it exists; and the stored shift is the stated rule.  tests/test_gpu_receding.py holds the device against the same files."""
import os

import numpy as np
import pytest

from conftest import golden
from oracle.harness import lib_path
from receding_cases import CASES, case, chain


def assert_same(got, want):
    for k in got:
        assert np.array_equal(np.asarray(got[k]), want[k]), k


@pytest.mark.parametrize("name", CASES)
def test_oracle_chain_equals_the_fixture(oracle_built, name):
    c = case(name)
    assert_same(chain(lib_path("oracle", c["problem"], c["fd"]), c), golden("receding_%s.npz" % name))
    ref = lib_path("ref", c["problem"], c["fd"])
    if os.path.exists(ref):  # the reference build's chain equals them too, where it exists
        assert_same(chain(ref, c), golden("receding_%s.npz" % name))


@pytest.mark.parametrize("name", CASES)
def test_fixture_shift_is_the_stated_rule(name):
    g = golden("receding_%s.npz" % name)
    s, x, u, us = int(g["s"]), g["plan_x"], g["plan_u"], g["shift_u"]
    n = u.shape[1]
    assert s == case(name)["s"] and 0 < s < n
    assert np.array_equal(us[:, :n - s], u[:, s:])                                   # u'[k] == u[k + s]
    assert np.array_equal(us[:, n - s:], np.repeat(u[:, -1:], s, axis=1))            # the tail holds u[N-1]
    assert np.array_equal(g["shift_x0"], x[:, s])                                    # x0' == x[s]
    assert np.array_equal(g["init_x"][:, 0], g["shift_x0"]) and np.all(g["init_ok"] == 1)
    # the plan's controls are within the limits already: for constant limits the initial roll-out's clamp changes nothing
    if name in ("carparking", "synth16x8", "almix"):
        assert np.array_equal(g["init_u"], us)
    # a warm start needs fewer iterations than the cold one did (the reason for the feature)
    assert np.median(g["warm_iters"]) < np.median(g["plan_iters"])
