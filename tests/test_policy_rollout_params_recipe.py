"""What tests/test_gpu_policy_rollout_params.py compares policy_rollout(params=...) against, checked without a GPU: the
oracle driver's forward_pass (tests/policy_cases.py reference_rollout) under every roll-out's own parameter dict
(tests/policy_param_cases.py), on the oracle build and, where it exists, bit for bit on the reference build.  A plan of the
NOMINAL parameters, rolled out under the draws: every reference roll-out is finite with ok = 1, perturbed limits keep
lower < upper, row r = 0 (the nominal values) gives the nominal-parameter roll-out bit for bit, and at least one other row
differs in cost from the nominal-parameter roll-out of the same start — the draws are no no-op.  Passes without the
feature: it keeps the GPU comparison honest."""
import os

import numpy as np
import pytest

from oracle.harness import lib_path
from policy_cases import cpu_plan, perturbed_starts, reference_rollout
from policy_param_cases import NAMED, R, SCALE, draws, limits_ordered, params_of, width
from test_policy_rollout_recipe import problem

KINDS = [(1.0, 1), (0.0, 0), (0.0, 1), (0.25, 0)]


@pytest.mark.parametrize("name,iterations", [("carparking", 7), ("synth16x8", 7)])
def test_reference_rollouts_under_the_draws_are_finite_and_differ(oracle_built, name, iterations):
    prob, fd, N, params, x0, u0 = problem(name)
    oracle, ref = lib_path("oracle", prob, fd), lib_path("ref", prob, fd)
    plan = cpu_plan(oracle, N, params, {}, x0, u0, iterations)
    starts = perturbed_starts(x0[None], R, seed=31)[0]
    table = draws(params, NAMED[name], 1, R, scale=SCALE[name])
    assert width(params, NAMED[name]) == {"carparking": 9, "synth16x8": 19}[name]
    assert limits_ordered(table)
    for n in NAMED[name]:
        assert np.array_equal(table[n][0, 0], np.asarray(params[n], dtype=np.float64)) and not np.array_equal(table[n][0, 1], table[n][0, 0])
    kw = dict(cost=plan["cost"], w_pen=plan["w_pen"], multipliers=plan["multipliers"])
    differ = 0
    for alpha, feedback in KINDS:
        for r in range(R):
            mine = params_of(params, table, 0, r)
            ok, c, x, u = reference_rollout(oracle, N, mine, {}, starts[r], plan["policy"], alpha, feedback, **kw)
            assert ok == 1 and np.isfinite(c) and np.all(np.isfinite(x)) and np.all(np.isfinite(u)), (alpha, feedback, r)
            ok0, c0, x0n, u0n = reference_rollout(oracle, N, params, {}, starts[r], plan["policy"], alpha, feedback, **kw)
            if r == 0:  # the nominal values, bit for bit
                assert (ok, c) == (ok0, c0) and np.array_equal(x, x0n) and np.array_equal(u, u0n), (alpha, feedback)
            else:
                differ += int(c != c0)
            if os.path.exists(ref):  # the reference's own forward_pass, where its build exists
                ok2, c2, x2, u2 = reference_rollout(ref, N, mine, {}, starts[r], plan["policy"], alpha, feedback, **kw)
                assert ok2 == ok and c2 == c and np.array_equal(x2, x) and np.array_equal(u2, u), (alpha, feedback, r)
    assert differ >= 1, "no draw changes a cost: the GPU comparison would hold with the parameters ignored"
    print("%s: %d of %d roll-outs with r >= 1 differ in cost from the nominal-parameter roll-out" % (name, differ, len(KINDS) * (R - 1)))
