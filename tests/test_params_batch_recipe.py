"""What tests/test_gpu_params_batch.py compares BatchSolver.set_params_batch against, checked without a GPU: the oracle
driver's init, calc_derivs, back_pass and line_search under each compared slot's OWN parameter dict
(tests/params_batch_cases.py), for every lane-mapped build.  Every stage succeeds with finite results, perturbed limits keep
lower < upper, and for at least one slot the gains and the accepted cost differ from the nominal-parameter run — the draws are
no no-op.  For the compaction case (hxtest, B = 300, max_iter = 60, compact = 16 as in tests/test_gpu_solve.py) the oracle's
iteration counts under the draws imply a gather: at some poll (every 4th iteration) at least 16 and at most half of the slots
are live.  Passes without the feature: it keeps the GPU comparison honest."""
import numpy as np
import pytest

from oracle.harness import HX_N, HX_PARAMS, Driver, hx_inputs, lib_path
from params_batch_cases import CPU_BUILDS, SLOTS, B, dict_of, oracle_stages, rows, setup
from policy_param_cases import NAMED, limits_ordered


@pytest.mark.parametrize("name,fd", [(n, fd) for n, fd, _ in CPU_BUILDS])
def test_every_stage_under_each_slots_parameters_succeeds_and_differs(oracle_built, name, fd):
    problem, N, params, opts, x0, u0 = setup(name, fd)
    table, _ = rows(name, params)
    assert limits_ordered(table)
    for n in NAMED[name]:
        assert not np.array_equal(table[n][:, 1], table[n][:, 0])
    lib = lib_path("oracle", problem, fd)
    differ = 0
    for b in SLOTS:  # (no compared slot may be left out)
        mine = oracle_stages(lib, N, dict_of(params, table, b), opts, x0[b], u0[b])
        nominal = oracle_stages(lib, N, params, opts, x0[b], u0[b])
        what = "%s fd%d slot %d" % (name, fd, b)
        assert mine["init"] == 1 and mine["derivs"] == 1 and mine["bp_rc"] == 0, what
        # line_search returns "accepted"; where the nominal parameters' own first search rejects every step size (almix: its
        # first iteration is rejected and the weights raised, oracle/harness.py) success is that every roll-out is finite
        assert mine["accept"] == 1 or nominal["accept"] == 0, what
        assert np.all(mine["alpha_ok"] == 1), what
        for k in ("x", "u", "cost", "fin", "l", "L", "dV0", "dV1", "alpha_cost", "new_cost"):
            assert np.all(np.isfinite(mine[k])), (what, k)
        # (a record may hold infinities by construction — almix: the open sides of its one-sided bounds — under any parameters)
        by_construction = ~np.isfinite(nominal["rec"])
        assert np.array_equal(~np.isfinite(mine["rec"]), by_construction) and np.array_equal(mine["rec"][by_construction], nominal["rec"][by_construction]), what
        differ += int((not np.array_equal(mine["l"], nominal["l"])) and (not np.array_equal(mine["L"], nominal["L"])) and
                      mine["new_cost"] != nominal["new_cost"])
    assert differ >= 1, "no slot's gains and accepted cost change: the GPU comparison would hold with the rows ignored"
    print("%s fd%d: %d of %d slots differ in gains and accepted cost from the nominal-parameter run" % (name, fd, differ, len(SLOTS)))


def test_the_compaction_case_gathers_under_the_draws(oracle_built):
    Bc, max_iter, compact = 300, 60, 16
    x0, u0 = hx_inputs(Bc)
    table, _ = rows("hxtest", HX_PARAMS, batch=Bc)
    assert limits_ordered(table)
    its = np.zeros(Bc, dtype=int)
    for b in range(Bc):
        d = Driver(lib_path("oracle", "hxtest", 0), HX_N, dict_of(HX_PARAMS, table, b), dict(max_iter=max_iter))
        assert d.init(x0[b], u0[b]) == 1
        d.solve()
        its[b] = int(d.scalars()["iterations"])
        d.close()
    # live at the poll behind `it` iterations: a start whose solve counts n iterations was iterated n times and left in its
    # (n + 1)-th (iLQG.c:297-303, :331: the exits come before the count goes up; k_update counts the same way), so it is
    # live behind `it` iterations iff n >= it
    polls = range(4, max_iter, 4)
    live = [int((its >= it).sum()) for it in polls]
    assert any(compact <= n <= Bc // 2 for n in live), live
    print("hxtest B = %d: iterations %d .. %d, live at the polls %s" % (Bc, its.min(), its.max(), live))
