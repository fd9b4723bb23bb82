"""What tests/test_gpu_param_steps.py compares BatchSolver.set_param_steps_batch against, checked without a GPU: the oracle
driver's init, calc_derivs, back_pass, every step size's forward pass and line_search under each compared slot's OWN window of
the per-time-step parameter (tests/param_steps_cases.py), almix and brachi_hli with FULL_DDP 0 and 1.  At every compared slot
every stage succeeds with finite roll-outs, and the gains and the accepted cost differ from the nominal-window run — the rows
are no no-op.  almix's initial cost does not depend on `vref` (it enters through a constraint whose penalty is zero in the
initial roll-out); brachi_hli's does, by 0.3 to 0.9.  brachi_hli's first search may reject under the draws where the nominal
window accepts: success there is finite roll-outs.  For the compaction case (almix FULL_DDP 1, B = 300, the case's max_iter =
80, compact = 16) the oracle's iteration counts under the rows imply a gather: at some poll (every 4th iteration) at least 16
and at most half of the slots are live.  Passes without the feature: it keeps the GPU comparison honest."""
import numpy as np
import pytest

from oracle.harness import Driver, lib_path
from param_steps_cases import CPU_BUILDS, SLOTS, STEP_NAME, B, dict_of, oracle_stages, setup, step_rows


@pytest.mark.parametrize("name,fd", CPU_BUILDS)
def test_every_stage_under_each_slots_window_succeeds_and_differs(oracle_built, name, fd):
    N, params, opts, x0, u0 = setup(name)
    rows = step_rows(name, params)
    nominal_window = np.asarray(params[STEP_NAME[name]], dtype=np.float64)
    assert rows.shape == (B, N + 1) and np.unique(rows).size == rows.size and not np.any(rows == nominal_window[None, :])
    lib = lib_path("oracle", name, fd)
    gaps = []
    for b in SLOTS:  # (no compared slot is left out)
        mine = oracle_stages(lib, N, dict_of(name, params, rows, b), opts, x0[b], u0[b])
        nominal = oracle_stages(lib, N, params, opts, x0[b], u0[b])
        what = "%s fd%d slot %d" % (name, fd, b)
        assert mine["init"] == 1 and mine["derivs"] == 1 and mine["bp_rc"] == 0, what
        assert np.all(mine["alpha_ok"] == 1) and len(mine["alpha_ok"]) == 8, what
        for k in ("x", "u", "cost", "fin", "l", "L", "dV0", "dV1", "alpha_cost", "new_cost"):
            assert np.all(np.isfinite(mine[k])), (what, k)
        by_construction = ~np.isfinite(nominal["rec"])  # (almix: the open sides of its one-sided bounds, under any parameters)
        assert np.array_equal(~np.isfinite(mine["rec"]), by_construction), what
        assert not np.array_equal(mine["l"], nominal["l"]) and not np.array_equal(mine["L"], nominal["L"]), what
        assert mine["new_cost"] != nominal["new_cost"], what
        gaps.append(abs(mine["cost"] - nominal["cost"]))
        if name == "almix":
            assert mine["cost"] == nominal["cost"], what
        else:
            assert 0.25 <= gaps[-1] < 0.95, (what, gaps[-1])  # (0.3 to 0.9 to one digit: the smallest is 0.2997, slot 69)
    print("%s fd%d: initial cost apart from the nominal window's by %s" % (name, fd, ", ".join("%.3g" % g for g in gaps)))


def test_the_compaction_case_gathers_under_the_rows(oracle_built):
    Bc, compact = 300, 16
    N, params, opts, x0, u0 = setup("almix", Bc)
    max_iter = opts["max_iter"]
    assert max_iter == 80
    rows = step_rows("almix", params, Bc)
    its = np.zeros(Bc, dtype=int)
    for b in range(Bc):
        d = Driver(lib_path("oracle", "almix", 1), N, dict_of("almix", params, rows, b), opts)
        assert d.init(x0[b], u0[b]) == 1
        d.solve()
        its[b] = int(d.scalars()["iterations"])
        d.close()
    # live at the poll behind `it` iterations: a start whose solve counts n iterations was iterated n times and left in its
    # (n + 1)-th, so it is live behind `it` iterations iff n >= it (tests/test_params_batch_recipe.py)
    live = [int((its >= it).sum()) for it in range(4, max_iter, 4)]
    assert any(compact <= n <= Bc // 2 for n in live), live
    print("almix B = %d: iterations %d .. %d, live at the polls %s" % (Bc, its.min(), its.max(), live))
