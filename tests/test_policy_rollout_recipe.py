"""What tests/test_gpu_policy_rollout.py compares BatchSolver.policy_rollout against, pinned to the reference's own sources
(no GPU): the driver recipe of tests/policy_cases.py — init from the start, set_state, set_gains, forward_pass, traj(1) —
gives the same bits on the reference build and on the CPU restatement, for all four (alpha, feedback) kinds; and the two
kinds the reference has no argument for ("l = 0, alpha = 1" for the pure feedback law, "L = 0" for the feed-forward step
alone) apply exactly the control the public header states."""
import os
import re

import numpy as np
import pytest

from conftest import ROOT, load_package
from oracle.harness import CAR_PARAMS, SYN_PARAMS_TIGHT, lib_path, syn_inputs
from policy_cases import COMBOS, cpu_plan, first_control, perturbed_starts, reference_rollout

R = 5


def problem(name):
    if name == "carparking":
        x0, u0 = load_package().synth.car_batch(1, 500, first=40)
        return "carparking", 0, 500, CAR_PARAMS, x0[0], u0[0]
    x0, u0 = syn_inputs(1, 12)
    return "synth16x8", 1, 12, SYN_PARAMS_TIGHT, x0[0], u0[0]


@pytest.mark.parametrize("name,iterations", [("carparking", 0), ("carparking", 7), ("synth16x8", 0), ("synth16x8", 7)])
def test_recipe_gives_the_reference_builds_bits(oracle_built, name, iterations):
    prob, fd, N, params, x0, u0 = problem(name)
    oracle, ref = lib_path("oracle", prob, fd), lib_path("ref", prob, fd)
    plan = cpu_plan(oracle, N, params, {}, x0, u0, iterations)
    starts = perturbed_starts(x0[None], R, seed=31, sigma=0.5 if name == "synth16x8" else 0.1)[0]
    kw = dict(cost=plan["cost"], w_pen=plan["w_pen"], multipliers=plan["multipliers"])
    clamped = 0
    for alpha, feedback in COMBOS:
        for r in range(R):
            ok, c, x, u = reference_rollout(oracle, N, params, {}, starts[r], plan["policy"], alpha, feedback, **kw)
            assert ok == 1 and np.isfinite(c) and np.all(np.isfinite(x)) and np.all(np.isfinite(u))
            assert np.array_equal(x[0], starts[r])
            # the first control is the stated formula, clamped: where the clamp is idle the bits are those of numpy
            want = first_control(plan["policy"], starts[r], alpha, feedback)
            lim = np.asarray(params["limW"] + params["limA"]).reshape(2, 2) if name == "carparking" else np.tile(params["lim"], (8, 1))
            inside = (want > lim[:, 0]) & (want < lim[:, 1])
            assert np.array_equal(u[0][inside], want[inside]), (alpha, feedback, r)
            assert np.array_equal(u[0][~inside], np.clip(want, lim[:, 0], lim[:, 1])[~inside])
            clamped += int(np.sum(~inside))
            if r == 0 and alpha == 0.0:  # the plan's own start without a feed-forward step: the plan again
                assert np.array_equal(u, plan["policy"][1]) and np.array_equal(x, plan["policy"][0])
            if os.path.exists(ref):  # the reference's own forward_pass, where its build exists
                ok2, c2, x2, u2 = reference_rollout(ref, N, params, {}, starts[r], plan["policy"], alpha, feedback, **kw)
                assert ok2 == ok and c2 == c and np.array_equal(x2, x) and np.array_equal(u2, u), (alpha, feedback, r)
    print("%s after %d iterations: %d first controls on a limit" % (name, iterations, clamped))


def test_public_header_states_what_the_recipe_pins():
    text = open(os.path.join(ROOT, "include", "ilqg_batch.h")).read()
    for entry in ("ilqg_batch_policy_rollout", "ilqg_batch_policy_rollout_device", "ilqg_multi_policy_rollout"):
        assert re.search(r"\bint %s\(" % entry, text), entry
    flat = " ".join(text.split())
    assert "u_k = u_nom_k [+ alpha * l_k if alpha != 0] [+ L_k (x_k - x_nom_k) if feedback]" in flat
    assert "PREVIOUS NOMINAL TRAJECTORY" in flat  # the gains behind an accepted step
    ilqg = load_package().ilqg
    assert "previous" in ilqg.BatchSolver.policy_rollout.__doc__.lower()
