"""What tests/test_gpu_receding_plant.py and tests/test_gpu_params_batch.py hold receding_plant's x, u, applied cost and x_plant
against, checked without a GPU: policy_cases.reference_plant, the reference's forward_pass one step at a time under the plant's
parameter dict, on the oracle build and, where it exists, with equal bits on the reference build.

For every build, slot, feedback value and step count the GPU tests compare (tests/plant_cases.py; the plan is the driver's own,
two iterations old — four in the per-trajectory cases —, as the batch's is):
  - the step costs forward_pass leaves behind (Driver.step_costs), summed in step order from 0.0, are its total bit for bit;
  - the chain without a disturbance is the first `steps` steps of ONE forward_pass bit for bit — x, u, step costs and the
    state behind them —, also at steps = n_hor - 1 on the short horizon: evaluating every step at time index 0 about the
    shifted policy changes nothing in these builds (none reads the time index outside a per-time-step parameter);
  - every compared reference value is finite (no compared slot may be left out);
  - three WRONG references miss the GPU tests' bar, 1e-10 max(1, |ref|), by at least 1e4 times in every compared slot:
    the cost under the model's parameters instead of the plant's, the disturbance of the steps before the last one dropped,
    and the trajectory's row put on top of the plant's for the parameter both name.  A kernel with one of these errors
    cannot pass the GPU tests by the reference's leniency.
Passes without the product: it keeps the GPU comparison honest."""
import os

import numpy as np
import pytest

from oracle.harness import Driver, lib_path
from plant_cases import SHORT_N, SLOTS, CpuCase, model_and_plant, noise, plant_starts
from policy_cases import cpu_plan, reference_plant, reference_rollout

BAR = 1e-10
MARGIN = 1e4 * BAR  # a wrong reference must be off by at least this much, relative to max(1, |ref|)

# (label, build, horizon, kind of plant, iterations of the plan, [(steps, dense disturbance)]): what the GPU tests compare
CASES = [
    ("carparking", "carparking", None, "shared", 2, [(3, False), (4, True), (2, True)]),   # (carparking_wave and the FMA-free build: the same problem)
    ("hxtest", "hxtest", None, "shared", 2, [(3, False), (4, True)]),
    ("synth16x8", "synth16x8", None, "shared", 2, [(3, False), (4, True), (2, True)]),
    ("synth10hx", "synth10hx", None, "shared", 2, [(3, False), (4, True)]),
    ("carparking n_hor=%d" % SHORT_N, "carparking", SHORT_N, "shared", 2, [(SHORT_N - 1, True), (1, True)]),
    ("carparking rows", "carparking", None, "rows", 4, [(3, True)]),
    ("hxtest rows", "hxtest", None, "rows", 4, [(3, True)]),
]


def gap(wrong, right):
    wrong, right = np.asarray(wrong, dtype=np.float64), np.asarray(right, dtype=np.float64)
    return float(np.max(np.abs(wrong - right) / np.maximum(1.0, np.abs(right))))


def same(a, b):
    return all(np.array_equal(np.asarray(p), np.asarray(q)) for p, q in zip(a, b))


@pytest.mark.parametrize("label,name,n_hor,kind,iterations,runs", CASES, ids=[c[0] for c in CASES])
def test_the_chain_is_the_references_roll_out_and_wrong_references_miss_the_bar(oracle_built, label, name, n_hor, kind, iterations, runs):
    c = CpuCase(name, n_hor)
    oracle, ref = lib_path("oracle", c.problem, c.fd), lib_path("ref", c.problem, c.fd)
    d = Driver(oracle, c.N)
    declared = d.param_desc()
    d.close()
    model, plant, swapped, _ = model_and_plant(c, kind, declared)
    X = plant_starts(c)
    smallest = {}

    def miss(key, value, what):
        smallest[key] = min(smallest.get(key, (np.inf, "")), (value, what))

    for s in SLOTS:
        plan = cpu_plan(oracle, c.N, model(s), c.opts, c.x0[s], c.u0[s], iterations)
        kw = dict(cost=plan["cost"], w_pen=plan["w_pen"], multipliers=plan["multipliers"])
        for feedback in (1, 0):
            for steps, dense in runs:
                what = "%s slot %d feedback=%d steps=%d" % (label, s, feedback, steps)
                w = noise(c, steps, rounds=1, last_only=not dense)[s]

                def chain(lib, params, w):
                    return reference_plant(lib, c.N, params, c.opts, X[s], plan["policy"], feedback, steps, w=w, **kw)

                # one forward_pass: its step costs add up to its total, and the chain without a disturbance is its first steps
                ok, total, xr, ur, sc = reference_rollout(oracle, c.N, plant(s), c.opts, X[s], plan["policy"], 0.0, feedback, step_costs=True, **kw)
                assert ok == 1 and np.all(np.isfinite(sc)), what
                acc = 0.0
                for v in sc:
                    acc += v
                assert acc == total, "%s: the step costs sum to %r, forward_pass returned %r" % (what, acc, total)
                x, u, cs, cost, x_end = chain(oracle, plant(s), None)
                assert np.array_equal(x, xr[:steps]) and np.array_equal(u, ur[:steps]) and np.array_equal(cs, sc[:steps]) and np.array_equal(x_end, xr[steps]), \
                    what + ": the chain of one-step roll-outs is not the roll-out"
                # what the GPU test compares: finite, and the reference build's bits
                right = chain(oracle, plant(s), w)
                assert all(np.all(np.isfinite(v)) for v in right), what + ": the reference is not finite (a compared slot may not be left out)"
                if os.path.exists(ref):
                    assert same(chain(ref, plant(s), w), right) and same(chain(ref, plant(s), None), (x, u, cs, cost, x_end)), what + ": the reference build's bits differ"
                    assert same(reference_rollout(ref, c.N, plant(s), c.opts, X[s], plan["policy"], 0.0, feedback, step_costs=True, **kw), (ok, total, xr, ur, sc)), what
                x, u, cs, cost, x_end = right
                # 1. the applied cost under the model's parameters
                miss("cost under the model's parameters", gap(chain(oracle, model(s), w)[3], cost), what)
                # 2. the disturbance of the steps before the last one dropped
                if dense and steps > 1:
                    w_last = w.copy()
                    w_last[:-1] = 0.0
                    x2, u2, _, cost2, xe2 = chain(oracle, plant(s), w_last)
                    miss("inner disturbance dropped: x", gap(x2, x), what)
                    miss("inner disturbance dropped: cost", gap(cost2, cost), what)
                    miss("inner disturbance dropped: x_plant", gap(xe2, x_end), what)
                    if feedback:
                        miss("inner disturbance dropped: u under feedback", gap(u2, u), what)
                # 3. the trajectory's row on top of the plant's
                if swapped is not None:
                    # (a weight of the running cost moves the cost alone where there is no feedback: one compared value off
                    # the bar fails the GPU test, so the largest of the four counts)
                    x3, u3, _, cost3, xe3 = chain(oracle, swapped(s), w)
                    miss("the trajectory's row on top: largest of x, u, cost, x_plant", max(gap(x3, x), gap(u3, u), gap(cost3, cost), gap(xe3, x_end)), what)
    print("%s: smallest gap of a wrong reference over slots, feedback values and step counts (the margin is %.3g): " % (label, MARGIN) +
          ", ".join("%s %.3g" % (k, v) for k, (v, _) in smallest.items()))
    for key, (value, what) in smallest.items():
        assert value >= MARGIN, "%s: the wrong reference (%s) is off by %.3g only, less than %.3g" % (what, key, value, MARGIN)
