"""What tests/test_gpu_policy_noise.py holds policy_rollout(disturbance=...) against, checked without a GPU:
policy_noise_cases.reference_disturbed_rollout, the reference's forward_pass one step at a time with the disturbance behind each
step, on the oracle build and on the reference build.

For every build the GPU test uses (its seven BUILDS are five problems), both histories (the plan is the driver's own: "fresh" =
init, calc_derivs, back_pass; "mid" = seven iterations, as the batch's is), every compared slot, kind and roll-out:
  - with a zero table (and with none) the chain is ONE whole forward_pass over the full horizon bit for bit — x, u, every step
    cost, the final cost and the total; in almix that holds the moved vref window and the moved running multipliers too;
  - every compared reference value is finite and ok = 1 (no compared roll-out may be left out);
  - the bar of the GPU test, 1e-10 max(1, |ref|), is attainable: the oracle build and the reference build agree within it on
    every compared roll-out, and for CarParking FULL_DDP 0 so does the reference build with FMA contraction;
  - the chain, which keeps one driver open, has the bits of the chain of policy_cases.reference_rollout calls, a driver per leg;
  - three WRONG recipes miss that bar by at least 1e4 times in every slot they are tried in: the table moved by one row, one
    row dropped, and the full table read as a shared one (roll-out (b, r) under row (0, r); the same confusion as a shared
    table read as a full one, whose rows of b > 0 lie behind the table's end).
The compared tables have a zero last row: the reference has no final cost at a state it did not reach itself.
Passes without the product: it keeps the GPU comparison honest."""
import os

import numpy as np
import pytest

from oracle.harness import lib_path
from plant_cases import SLOTS, CpuCase
from policy_cases import cpu_plan, perturbed_starts, reference_rollout
from policy_noise_cases import KINDS, R, leg_by_leg, reference_disturbed_rollout, step_params, tables, worst

BAR = 1e-10
MARGIN = 1e4 * BAR
PROBLEMS = ["carparking", "hxtest", "synth16x8", "synth10hx", "almix"]


def same(a, b):
    return all(np.array_equal(np.asarray(p), np.asarray(q)) for p, q in zip(a, b))


@pytest.mark.parametrize("kind", ["fresh", "mid"])
@pytest.mark.parametrize("name", PROBLEMS)
def test_the_chain_is_the_references_roll_out_and_wrong_recipes_miss_the_bar(oracle_built, name, kind):
    c = CpuCase(name)
    oracle, ref = lib_path("oracle", c.problem, c.fd), lib_path("ref", c.problem, c.fd)
    others = [p for p in (ref, lib_path("ref_fma", c.problem, c.fd)) if os.path.exists(p)]
    moving = step_params(oracle, c.N)
    assert moving == (["vref"] if name == "almix" else [])
    starts = perturbed_starts(c.x0, R, seed=17)
    W = tables(c)
    assert not np.any(W[:, 0]) and not np.any(W[:, :, -1]) and np.all(np.any(W[:, 1:, :-1] != 0.0, axis=(2, 3)))
    smallest, between = {}, 0.0

    def miss(key, value, what):
        smallest[key] = min(smallest.get(key, (np.inf, "")), (value, what))

    def gap(a, b):  # (ok, cost, x, u, c): the largest of what the GPU test compares
        return max(worst(a[1], b[1]), worst(a[2], b[2]), worst(a[3], b[3]))

    for s in SLOTS:
        plan = cpu_plan(oracle, c.N, c.params, c.opts, c.x0[s], c.u0[s], 0 if kind == "fresh" else 7)
        kw = dict(cost=plan["cost"], w_pen=plan["w_pen"], multipliers=plan["multipliers"])
        for alpha, feedback in KINDS:
            def chain(lib, r, w):
                return reference_disturbed_rollout(lib, c.N, c.params, c.opts, starts[s, r], plan["policy"], alpha, feedback, w=w, moving=moving, **kw)

            for r in range(R):
                what = "%s %s slot %d alpha=%g feedback=%d roll-out %d" % (name, kind, s, alpha, feedback, r)
                right = chain(oracle, r, W[s, r])
                assert right[0] == 1 and all(np.all(np.isfinite(v)) for v in right[1:]), what + ": the reference is not finite"
                acc = 0.0
                for v in right[4]:
                    acc += v
                assert acc == right[1], what
                for lib in others:
                    other = chain(lib, r, W[s, r])
                    assert other[0] == 1, what
                    between = max(between, gap(other, right))
                    assert gap(other, right) <= BAR, "%s: %s is %.3g from the oracle build: the bar is not attainable" % (what, os.path.basename(lib), gap(other, right))
                if r <= 1:  # a zero table, and none: one whole forward_pass, bit for bit (r = 0: the plan's own start)
                    whole = reference_rollout(oracle, c.N, c.params, c.opts, starts[s, r], plan["policy"], alpha, feedback, step_costs=True, **kw)
                    for w in (np.zeros((c.N, c.nx)), None):
                        assert same(chain(oracle, r, w), whole), what + ": the chain with a zero table is not the forward_pass"
                    if os.path.exists(ref):
                        assert same(chain(ref, r, None), reference_rollout(ref, c.N, c.params, c.opts, starts[s, r], plan["policy"], alpha, feedback,
                                                                           step_costs=True, **kw)), what + ": on the reference build"
                if r == 0:
                    assert same(right, whole), what
                if r == 1 and s == SLOTS[-1]:  # the chain in one driver is the chain of reference_rollout calls
                    assert same(leg_by_leg(oracle, c.N, c.params, c.opts, starts[s, r], plan["policy"], alpha, feedback, w=W[s, r], moving=moving, **kw),
                                right), what + ": one driver for the chain against one per leg"
                if r == 1:
                    moved = np.concatenate([W[s, r][1:], np.zeros((1, c.nx))])
                    miss("the table moved by one row", gap(chain(oracle, r, moved), right), what)
                    dropped = W[s, r].copy()
                    dropped[c.N // 2] = 0.0
                    miss("row n_hor / 2 dropped", gap(chain(oracle, r, dropped), right), what)
                    if s != 0:
                        miss("the full table read as a shared one", gap(chain(oracle, r, W[0, r]), right), what)
    print("%s %s: oracle and reference builds within %.3g of each other; smallest gap of a wrong recipe over slots and kinds (the margin is %.3g): "
          % (name, kind, between, MARGIN) + ", ".join("%s %.3g" % (k, v) for k, (v, _) in smallest.items()))
    assert len(smallest) == 3
    for key, (value, what) in smallest.items():
        assert value >= MARGIN, "%s: the wrong recipe (%s) is off by %.3g only, less than %.3g" % (what, key, value, MARGIN)
