"""What tests/test_gpu_receding_windows.py holds the resident loops with moving windows against, checked without a GPU, on the
oracle build and, where it exists, on the reference build (the cases are those of tests/window_loop_cases.py).  Three
conditions keep the GPU comparison honest; a loop that forgot to move a window, or a plant that read every step's value at
time index 0, cannot pass by the reference's leniency:

  (a) the model loop (brachi_hli, FULL_DDP 0 and 1, rows, iterations = 0): from round 1 on the cost of the initial roll-out
      under the MOVED window and under the UNMOVED one differ by at least 1e4 bars at every compared slot (a bar is
      1e-10 max(1, |ref|), what the GPU test allows);
  (b) the plant loop (almix, FULL_DDP 1, feedback): the chain of one-step roll-outs with the window shifted by k at step k
      (window_loop_cases.plant_chain) is, without a disturbance, the first `steps` steps of ONE forward_pass under the round's
      window bit for bit — states, controls, step costs and the state behind them;
  (c) the same chain with the window kept where it is (every step reads time index 0) misses the applied cost by at least 1e4
      bars at every compared slot, in every one of the three rounds (in almix only the cost depends on `vref`: the states and
      controls of the two chains are the same).
The rounds follow each other as in the loop: the plan of round r + 1 starts from the state the plant reached, with the controls
shifted by `steps` and the last one held, under the window moved by `steps`.  Passes without the feature."""
import os

import numpy as np
import pytest

from oracle.harness import Driver, lib_path
from policy_cases import cpu_plan, reference_rollout, shifted
from window_loop_cases import ITERATIONS, ROUNDS, SLOTS, STEPS, B, bars, dict_at, noise, plant_chain, plant_starts, setup, track

MARGIN = 1e4  # bars


def libs(name, fd):
    ref = lib_path("ref", name, fd)
    return [("oracle", lib_path("oracle", name, fd))] + ([("reference", ref)] if os.path.exists(ref) else [])


@pytest.mark.parametrize("fd", [0, 1])
def test_a_moved_window_and_an_unmoved_one_are_far_apart_in_the_model_loop(oracle_built, fd):
    name = "brachi_hli"
    N, params, opts, x0, u0 = setup(name)
    T = track(name, params, N)
    assert T.shape == (B, N + 1 + ROUNDS * STEPS) and np.unique(T).size == T.size
    for kind, lib in libs(name, fd):
        smallest = np.inf
        for b in SLOTS:
            start = x0[b]
            for r in range(ROUNDS):
                u = shifted(u0[b], r * STEPS)
                costs = []
                for at in (r * STEPS, 0):
                    d = Driver(lib, N, dict_at(name, params, T, N, b, at), opts)
                    assert d.init(start, u) == 1, (kind, b, r, at)
                    costs.append(d.scalars()["cost"])
                    if at == r * STEPS:
                        x, _ = d.traj(0)
                    d.close()
                assert np.isfinite(costs[0]) and np.all(np.isfinite(x)), (kind, b, r)
                if r >= 1:
                    smallest = min(smallest, bars(costs[1], costs[0]))
                    assert bars(costs[1], costs[0]) >= MARGIN, "%s fd%d slot %d round %d: the unmoved window is off by %.3g bars only" % (
                        kind, fd, b, r, bars(costs[1], costs[0]))
                start = x[STEPS]
        print("brachi_hli fd%d, %s build: the cost under the unmoved window misses by at least %.3g bars" % (fd, kind, smallest))


def test_the_plant_chain_is_the_references_roll_out_and_time_index_zero_misses_the_cost(oracle_built):
    name, fd = "almix", 1
    N, params, opts, x0, u0 = setup(name)
    T = track(name, params, N)
    assert T.shape == (B, N + 1 + ROUNDS * STEPS) and np.unique(T).size == T.size
    X = plant_starts(x0)
    w = noise(x0.shape[1], STEPS)
    for kind, lib in libs(name, fd):
        smallest = {r: np.inf for r in range(ROUNDS)}
        for b in SLOTS:
            start, u, xp = x0[b], u0[b], X[b]
            for r in range(ROUNDS):
                at = r * STEPS
                what = "%s slot %d round %d" % (kind, b, r)
                plan = cpu_plan(lib, N, dict_at(name, params, T, N, b, at), opts, start, u, ITERATIONS)
                kw = dict(cost=plan["cost"], w_pen=plan["w_pen"], multipliers=plan["multipliers"])
                args = (lib, name, N, params, T, b, at, opts, xp, plan["policy"], 1, STEPS)
                # (b) without a disturbance the chain is one forward_pass under the round's window
                ok, _, xr, ur, sc = reference_rollout(lib, N, dict_at(name, params, T, N, b, at), opts, xp, plan["policy"], 0.0, 1, step_costs=True, **kw)
                assert ok == 1 and np.all(np.isfinite(sc)), what
                xs, us, cs, _, x_end = plant_chain(*args, w=None, **kw)
                assert np.array_equal(xs, xr[:STEPS]) and np.array_equal(us, ur[:STEPS]) and np.array_equal(cs, sc[:STEPS]) and \
                    np.array_equal(x_end, xr[STEPS]), what + ": the chain with shifted windows is not the roll-out"
                # (c) every step at time index 0 misses the applied cost, and nothing else
                right = plant_chain(*args, w=w[b, at:at + STEPS], **kw)
                wrong = plant_chain(*args, w=w[b, at:at + STEPS], moving=False, **kw)
                assert all(np.all(np.isfinite(v)) for v in right), what + ": the reference is not finite (a compared slot may not be left out)"
                assert np.array_equal(wrong[0], right[0]) and np.array_equal(wrong[1], right[1]) and np.array_equal(wrong[4], right[4]), what
                miss = bars(wrong[3], right[3])
                smallest[r] = min(smallest[r], miss)
                assert miss >= MARGIN, "%s: the chain at time index 0 misses the applied cost by %.3g bars only" % (what, miss)
                # the next round: the plan shifts onto the plant's state, the window has moved
                start, u, xp = right[4], shifted(plan["policy"][1], STEPS), right[4]
        print("almix fd1, %s build: the applied cost at time index 0 misses by at least %s bars (rounds 0, 1, 2)" % (
            kind, ", ".join("%.3g" % smallest[r] for r in range(ROUNDS))))
