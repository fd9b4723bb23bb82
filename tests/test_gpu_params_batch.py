"""BatchSolver.set_params_batch on the GPU: every trajectory of a batch plans under problem parameters of its own (the
instantiations of k_rollout, k_derivs_rows, k_backward, k_search, k_multipliers_rows, k_policy and k_plant that take the table).

Cases are those of tests/params_batch_cases.py (B = 70, SLOTS 0, 63, 64, 69; 5 % draws, row [:, 1] = trajectory b's row;
lane-mapped builds), which tests/test_params_batch_recipe.py shows to be no no-op on the CPU.  Test 1 holds every stage against
the oracle driver under THAT slot's parameter dict with the tree's single-pass bar |d| <= 1e-10 max(1, |ref|); the other tests
are identities between calls of the product and are bit for bit unless they say otherwise."""
import numpy as np
import pytest

from oracle.harness import HX_N, HX_PARAMS, hx_inputs, lib_path
from params_batch_cases import BUILDS, SLOTS, B, FdCase, dict_of, oracle_stages, rows, setup
from plant_cases import BOTH, noise, plant_over_rows, plant_starts
from policy_cases import perturbed_starts, reference_rollout
from policy_param_cases import NAMED, PER_STEP, draws, params_of
from test_gpu_policy_rollout import close, ilqg, outputs_equal, torch, worst  # noqa: F401 (fixtures)
from test_gpu_receding_plant import composition, full_state, hold_rounds

pytestmark = pytest.mark.gpu

_ORACLE = {}


def oracle(c, table, b, opts=None):
    """the oracle's stages for slot b under its own dict, computed once per (build, slot) and shared"""
    key = (c.problem, c.fd, b, tuple(sorted((opts or {}).items())))
    if key not in _ORACLE:
        _ORACLE[key] = oracle_stages(lib_path("oracle", c.problem, c.fd), c.N, dict_of(c.params, table, b), dict(c.opts, **(opts or {})), c.x0[b], c.u0[b])
    return _ORACLE[key]


def states_equal(a, b, what, rows_a=slice(None), rows_b=slice(None)):
    for k in a:
        assert np.array_equal(np.asarray(a[k])[rows_a], np.asarray(b[k])[rows_b]), "%s: %s differs" % (what, k)


def close_inf(got, want):
    """close() where the reference is finite, equal where it holds an infinity by construction (almix's one-sided bounds)"""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    fin = np.isfinite(want)
    return close(got[fin], want[fin]) and np.array_equal(got[~fin], want[~fin])


def launches(s):
    return {k: n for k, (n, _) in s.kernel_times().items()}


# ---------------------------------------------------------------------------
# 1. stage by stage against the reference
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("name,fd,strict", BUILDS)
def test_every_stage_equals_the_oracle_under_the_slots_own_parameters(ilqg, name, fd, strict):
    c = FdCase(ilqg, name, fd, strict, count=2, opts=dict(ls_split=0))  # (ls_split = 0: every step size is rolled out for every slot)
    s, fused = c.solvers
    table, mine = rows(name, c.params)
    dev = {}

    def hold(key, got, want, b):
        dev[key] = max(dev.get(key, 0.0), worst(np.asarray(got)[np.isfinite(want)], np.asarray(want)[np.isfinite(want)]))
        assert close_inf(got, want), "%s fd%d slot %d: %s off by %.3g" % (name, fd, b, key, dev[key])

    for q in (s, fused):
        q.set_params_batch(mine)
        q.init(c.x0, c.u0)
    x, cost = s.x(), s.scalar("cost")
    for b in SLOTS:
        ref = oracle(c, table, b)
        assert ref["init"] == 1 and s.ints("status")[b] == 0
        hold("x", x[b], ref["x"], b)
        hold("cost", cost[b], ref["cost"], b)
    s.calc_derivs()
    rec, fin = s.derivs()
    nd = s.problem.rec_dev
    for b in SLOTS:
        ref = oracle(c, table, b)
        hold("records", rec[b][:, :nd], ref["rec"][:, :nd], b)
        hold("final record", fin[b], ref["fin"], b)
    s.back_pass(single_sweep=True)
    fused.back_pass(fused=True)
    for tag, q in (("", s), ("fused ", fused)):
        l, L = q.gains()
        dV0, dV1, rc = q.scalar("dV0"), q.scalar("dV1"), q.ints("bp_rc")
        for b in SLOTS:
            ref = oracle(c, table, b)
            assert rc[b] == ref["bp_rc"] == 0
            hold(tag + "l", l[b], ref["l"], b)
            hold(tag + "L", L[b], ref["L"], b)
            hold(tag + "dV", [dV0[b], dV1[b]], [ref["dV0"], ref["dV1"]], b)
    s.line_search()
    ac, ok, idx, acc = s.scalar("alpha_cost"), s.ints("alpha_ok"), s.ints("alpha_idx"), s.ints("accepted")
    for b in SLOTS:
        ref = oracle(c, table, b)
        na = len(ref["alpha_cost"])
        assert np.array_equal(ok[b][:na], ref["alpha_ok"]) and acc[b] == ref["accept"] and idx[b] == ref["alpha_idx"], (name, fd, b)
        hold("alpha_cost", ac[b][:na], ref["alpha_cost"], b)
    print("%s fd%d%s: worst deviation from the oracle under the slots' own parameters: " % (name, fd, " FMA-free" if strict else "") +
          ", ".join("%s %.3g" % kv for kv in dev.items()))
    c.close()


# ---------------------------------------------------------------------------
# 2. a batch is its trajectories
# ---------------------------------------------------------------------------
def test_a_batch_is_its_trajectories(ilqg):
    """FMA-free CarParking, iterate(5): slot b of the per-trajectory batch has the bits of a batch of ONE trajectory whose
    shared parameters (set_param) are that slot's values"""
    c = FdCase(ilqg, "carparking", 0, True)
    (s,) = c.solvers
    table, mine = rows("carparking", c.params)
    s.set_params_batch(mine)
    s.init(c.x0, c.u0)
    s.iterate(5)
    whole = full_state(s)
    for b in SLOTS:
        one = ilqg.BatchSolver(c.problem, c.fd, batch=1, n_hor=c.N, params=c.params, opts=dict(c.opts, max_iter=40), strict=True)
        for n in NAMED["carparking"]:
            one.set_param(n, mine[n][b])
        one.init(c.x0[b:b + 1], c.u0[b:b + 1])
        one.iterate(5)
        states_equal(full_state(one), whole, "slot %d against a batch of one under set_param" % b, slice(0, 1), slice(b, b + 1))
        one.close()
    c.close()


def test_a_batch_is_its_trajectories_with_per_lane_loads_in_the_searches(ilqg, monkeypatch):
    """The same identity under ILQG_NO_DMA=1, short horizon: the searches then load the nominal records per lane
    (k_search<0 | 1, false>), a form the record size of no shipped lane-mapped problem selects, so its instantiations with the
    table are reached by nothing else.  FMA-free CarParking, B = 70, n_hor = 8, iterate(5), bit for bit."""
    N = 8
    monkeypatch.setenv("ILQG_NO_DMA", "1")  # (read when a context is created)
    problem, _, params, opts, x0, u0 = setup("carparking", 0)
    u0 = np.ascontiguousarray(u0[:, :N])
    kw = dict(n_hor=N, params=params, opts=dict(opts, max_iter=40), strict=True)
    s = ilqg.BatchSolver(problem, 0, batch=B, **kw)
    table, mine = rows("carparking", params)
    s.set_params_batch(mine)
    s.init(x0, u0)
    s.iterate(5)
    whole = full_state(s)
    for b in SLOTS:
        one = ilqg.BatchSolver(problem, 0, batch=1, **kw)
        for n in NAMED["carparking"]:
            one.set_param(n, mine[n][b])
        one.init(x0[b:b + 1], u0[b:b + 1])
        one.iterate(5)
        states_equal(full_state(one), whole, "slot %d against a batch of one under set_param, per-lane loads" % b, slice(0, 1), slice(b, b + 1))
        one.close()
    s.close()


# ---------------------------------------------------------------------------
# 3. nominal rows
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("name,fd,strict", BUILDS)
def test_nominal_rows_give_the_shared_batch(ilqg, name, fd, strict):
    """the batch's own values in every row of EVERY fixed-size parameter: bit for bit the shared batch after iterate(5) in
    the FMA-free build; in the product builds (the kernels that take the table are other code: other contractions) after one
    iteration within the single-pass bar"""
    c = FdCase(ilqg, name, fd, strict, count=2)
    shared, per = c.solvers
    fixed = [n for n, size in per.problem.params if size > 0]
    per.set_params_batch({n: np.broadcast_to(np.asarray(c.params[n], dtype=np.float64), (B, np.size(c.params[n]))) for n in fixed})
    for q in (shared, per):
        q.init(c.x0, c.u0)
        q.iterate(5 if strict else 1)
    a, b = full_state(shared), full_state(per)
    if strict:
        states_equal(b, a, "nominal rows against the shared batch")
    else:
        for k in a:
            if a[k].dtype.kind == "i":
                assert np.array_equal(a[k], b[k]), k
            else:
                assert close(b[k], a[k]), "%s off by %.3g" % (k, worst(b[k], a[k]))
    for n in fixed:
        assert np.array_equal(per.params_batch(n), shared.params_batch(n)) and np.array_equal(per.params_batch(n)[B - 1], np.asarray(c.params[n], dtype=np.float64))
    c.close()


# ---------------------------------------------------------------------------
# 4. identities within the new code
# ---------------------------------------------------------------------------
def mid_then_five(s, c, mine, setter=None, flip=False):
    (setter or s.set_params_batch)(mine)
    s.init(c.x0[::-1].copy() if flip else c.x0, c.u0[::-1].copy() if flip else c.u0)
    s.iterate(7)
    if c.name == "carparking":  # both locations occur: kept roll-out planes and X / U (tests/test_gpu_policy_rollout.py, history "mid")
        acc, idx = s.ints("accepted"), s.ints("alpha_idx")
        assert np.any((acc == 1) & (idx <= 4)) and np.any((acc == 0) | (idx > 4))
    s.iterate(5)
    return full_state(s)


@pytest.mark.parametrize("name,fd", [("carparking", 0), ("hxtest", 1), ("almix", 1)])
def test_identities_of_the_per_trajectory_batch(ilqg, torch, name, fd):
    c = FdCase(ilqg, name, fd, count=6)
    table, mine = rows(name, c.params)
    base = mid_then_five(c.solvers[0], c, mine)
    assert np.array_equal(c.solvers[0].params_batch(NAMED[name][0]), mine[NAMED[name][0]].reshape(B, -1))
    # the order of names
    states_equal(mid_then_five(c.solvers[1], c, {n: mine[n] for n in reversed(list(mine))}), base, "names in reverse order")
    # an extra named parameter at nominal values
    extra = next(n for n, size in c.solvers[0].problem.params if size > 0 and n not in mine)
    more = dict(mine, **{extra: np.broadcast_to(np.asarray(c.params[extra], dtype=np.float64), (B, np.size(c.params[extra])))})
    states_equal(mid_then_five(c.solvers[2], c, more), base, "an extra parameter at its nominal values")
    # host against device setter
    s = c.solvers[3]
    dev = {n: torch.tensor(a, dtype=torch.float64, device="cuda:0") for n, a in mine.items()}
    states_equal(mid_then_five(s, c, dev, lambda p: s.set_params_batch(p, device=True)), base, "device setter against host setter")
    # set, clear, set again
    s = c.solvers[4]
    s.set_params_batch(more)
    s.set_params_batch({})
    states_equal(mid_then_five(s, c, mine), base, "set, clear, set again")
    # the batch reversed together with its rows gives the reversed results
    s = c.solvers[5]
    got = mid_then_five(s, c, {n: a[::-1].copy() for n, a in mine.items()}, flip=True)
    states_equal({k: v[::-1] for k, v in got.items()}, base, "the reversed batch with reversed rows")
    c.close()


def test_groups_and_shards_hold_their_slices_of_the_rows(ilqg):
    """B = 200 is four stream groups of 64 (the last one ragged): groups 1 against 4, and three shards of a MultiSolver on
    one device, each with the rows from its first trajectory on"""
    n = 200
    cases = [FdCase(ilqg, "carparking", 0, groups=g, batch=n) for g in (1, 4)]
    c = cases[0]
    table, mine = rows("carparking", c.params, batch=n)
    outs = [mid_then_five(q.solvers[0], q, mine) for q in cases]
    states_equal(outs[1], outs[0], "four stream groups against one")
    m = ilqg.MultiSolver("carparking", 0, batch=n, n_hor=c.N, devices=[0] * 3, params=c.params, opts=dict(max_iter=40))
    m.set_params_batch(mine)
    m.init(c.x0, c.u0)
    m.iterate(12)
    assert np.array_equal(m.x(), outs[0]["x"]) and np.array_equal(m.u(), outs[0]["u"])
    assert np.array_equal(m.ints("iterations"), outs[0]["iterations"]) and np.array_equal(m.ints("status"), outs[0]["status"])
    m.close()
    for q in cases:
        q.close()


# ---------------------------------------------------------------------------
# 5. cleared means parent, and every refusal leaves it so (the refusals: test 9)
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("name,fd,strict", [("carparking", 0, False), ("almix", 1, False)])
def test_a_cleared_set_is_the_batch_that_never_had_one(ilqg, name, fd, strict):
    c = FdCase(ilqg, name, fd, strict, count=2)
    never, cleared = c.solvers
    table, mine = rows(name, c.params)
    cleared.set_params_batch(mine)
    cleared.init(c.x0, c.u0)
    cleared.iterate(2)
    cleared.set_params_batch({})
    for q in (never, cleared):
        q.init(c.x0, c.u0)
        q.iterate(5)
    states_equal(full_state(cleared), full_state(never), "set, iterate, clear, init against a batch without a table")
    cleared.set_param(NAMED[name][0], c.params[NAMED[name][0]])  # (shared again: set_param of that name is no longer refused)
    c.close()


# ---------------------------------------------------------------------------
# 6. compaction: the rows travel with their trajectories
# ---------------------------------------------------------------------------
def test_a_compacted_solve_equals_the_plain_one(ilqg):
    """the hxtest case of tests/test_gpu_solve.py (B = 300, max_iter = 60, compact = 16) under the draws (the recipe test: they
    imply a gather)"""
    n = 300
    x0, u0 = hx_inputs(n)
    table, mine = rows("hxtest", HX_PARAMS, batch=n)
    out = []
    for compact in (0, 16):
        s = ilqg.BatchSolver("hxtest", 0, batch=n, n_hor=HX_N, params=HX_PARAMS, opts=dict(max_iter=60, compact=compact))
        s.set_params_batch(mine)
        s.init(x0, u0)
        s.solve()
        l, L = s.gains()
        o = dict(x=s.x(), u=s.u(), l=l, L=L, trace=s.solve_trace())  # (the keys of _solve in tests/test_gpu_solve.py)
        for k in ("cost", "lambda", "dlambda", "g_norm", "dV0", "dV1", "new_cost", "dcost", "expected", "alpha_cost"):
            o[k] = s.scalar(k).copy()
        for k in ("status", "iterations", "alpha_idx", "accepted", "bp_calls", "alpha_ok"):
            o[k] = s.ints(k).copy()
        assert np.array_equal(s.params_batch("lim"), mine["lim"])  # (the caller's batch keeps its rows)
        out.append(o)
        s.close()
    plain, comp = out
    assert comp["trace"][3] >= 1 and plain["trace"][3] == 0, comp["trace"]
    for k in plain:
        if k != "trace":
            assert np.array_equal(plain[k], comp[k]), k


# ---------------------------------------------------------------------------
# 7. roll-outs and plant inherit the model
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("name,fd", [("carparking", 0), ("almix", 1)])
def test_policy_rollouts_run_under_the_trajectorys_parameters(ilqg, name, fd):
    R = 3
    c = FdCase(ilqg, name, fd)
    (s,) = c.solvers
    table, mine = rows(name, c.params)
    s.set_params_batch(mine)
    s.init(c.x0, c.u0)
    s.iterate(7)
    starts = perturbed_starts(c.x0, R, seed=17)
    plain = s.policy_rollout(starts, 1.0, True, trajectories=True)
    # one parameter that is also per-trajectory and one that is not; the roll-out's row goes on top of the trajectory's
    both = NAMED[name][0]
    other = next(n for n, size in s.problem.params if size > 0 and n not in mine)
    roll = draws(c.params, (both, other), B, R, seed=71)
    named = s.policy_rollout(starts, 1.0, True, trajectories=True, params=roll)
    h = s.head(c.N, gains=True)
    cost = s.scalar("cost")
    mul = sum(s.multiplier_dims()) > 0
    w_l, w_f = (s.scalar("w_pen_l"), s.scalar("w_pen_f")) if mul else (np.zeros(B), np.zeros(B))
    m_run, m_fin = s.multipliers() if mul else (None, None)
    lib = lib_path("oracle", c.problem, c.fd)
    dev = 0.0
    for b in SLOTS:
        policy = (h["x"][b], h["u"][b], h["l"][b], h["L"][b])
        kw = dict(cost=cost[b], w_pen=(w_l[b], w_f[b]), multipliers=(m_run[b], m_fin[b]) if mul else None)
        for r in range(R):
            for out, p in ((plain, dict_of(c.params, table, b)), (named, params_of(dict_of(c.params, table, b), roll, b, r))):
                ok, cr, xr, ur = reference_rollout(lib, c.N, p, c.opts, starts[b, r], policy, 1.0, 1, **kw)
                assert ok == 1 and out["ok"][b, r] == 1, (b, r)
                for got, want in ((out["cost"][b, r], cr), (out["x"][b, r], xr), (out["u"][b, r], ur), (out["x_end"][b, r], xr[-1])):
                    dev = max(dev, worst(got, want))
                    assert close(got, want), "%s slot %d start %d: off by %.3g" % (name, b, r, worst(got, want))
    print("%s: policy roll-outs under the trajectories' parameters, worst deviation from the oracle %.3g" % (name, dev))
    c.close()


def test_the_plant_without_names_is_the_trajectorys_model(ilqg):
    """receding_plant(n_names = 0) for one round = iterate + policy_rollout (R = 1, from the plan's x_0, alpha = 0, feedback) +
    shift composed; bit for bit in the FMA-free build"""
    steps, iters = 3, 4
    c = FdCase(ilqg, "carparking", 0, True, count=2)
    loop, comp = c.solvers
    table, mine = rows("carparking", c.params)
    for q in (loop, comp):
        q.set_params_batch(mine)
        q.init(c.x0, c.u0)
    log = loop.receding_plant(1, steps, iters, True)
    comp.iterate(iters)
    roll = comp.policy_rollout(c.x0[:, None], 0.0, True, trajectories=True)
    comp.shift(steps, x0=roll["x"][:, 0, steps])
    assert np.all(log["ok"] == 1) and np.all(roll["ok"] == 1)
    assert np.array_equal(log["x"], roll["x"][:, 0, :steps]) and np.array_equal(log["u"], roll["u"][:, 0, :steps])
    states_equal(full_state(loop), full_state(comp), "the loop against its composition")
    c.close()


@pytest.mark.parametrize("name,fd", [("carparking", 0), ("hxtest", 1)])
def test_the_plant_with_names_runs_over_the_trajectorys_row(ilqg, name, fd):
    """per-trajectory rows AND a plant with named parameters (k_plant<true> with both tables): one round of three steps behind
    four iterations, feedback, a disturbance behind every step.  The plant names one parameter the trajectories' rows name too
    and one they do not (tests/plant_cases.py); slot b's plant runs under the batch's parameters with the trajectory's row
    first and the plant's row on top.  x, u, the applied cost and x_plant against policy_cases.reference_plant under that
    dict (tests/test_plant_reference_recipe.py: the other order misses the bar by 1e4 times or more)."""
    steps, iters = 3, 4
    c = FdCase(ilqg, name, fd, count=2)
    loop, twin = c.solvers
    table, mine, plant_table, plant_rows = plant_over_rows(name, c.params, loop.problem.params)
    assert BOTH[name] in mine and BOTH[name] in plant_rows and sum(n not in mine for n in plant_rows) == 1
    for q in (loop, twin):
        q.set_params_batch(mine)
        q.init(c.x0, c.u0)
    X, w = plant_starts(c), noise(c, steps, rounds=1)
    out = loop.receding_plant(1, steps, iters, True, X, plant_rows, w)
    what = "%s fd%d, plant rows over trajectory rows" % (name, fd)
    dev = hold_rounds(c, out, twin, lambda b: params_of(dict_of(c.params, table, b), plant_table, b, 1), X, w, 1, steps, 1, what, iterations=iters)
    print(what + ": worst deviation from the reference's plant " + ", ".join("%s %.3g" % kv for kv in dev.items()))
    c.close()


def test_the_plant_with_names_over_rows_equals_its_composition(ilqg):
    """the same call in the FMA-free CarParking build, the disturbance behind the last step only, against iterate +
    policy_rollout(params = the plants' rows) on the same per-trajectory batch + shift: logs, x_plant and the batch, bit for bit"""
    steps, iters = 3, 4
    c = FdCase(ilqg, "carparking", 0, True, count=2)
    loop, comp = c.solvers
    table, mine, plant_table, plant_rows = plant_over_rows("carparking", c.params, loop.problem.params)
    for q in (loop, comp):
        q.set_params_batch(mine)
        q.init(c.x0, c.u0)
    X, w = plant_starts(c), noise(c, steps, rounds=1, last_only=True)
    out = loop.receding_plant(1, steps, iters, True, X, plant_rows, w)
    assert np.all(out["ok"] == 1)
    want = composition(comp, plant_rows, X, w, 1, steps, iterations=iters)
    outputs_equal(out, want, "plant rows over trajectory rows: one call against the composition, FMA-free build", sorted(want))
    states_equal(full_state(loop), full_state(comp), "plant rows over trajectory rows: the loop against its composition")
    c.close()


# ---------------------------------------------------------------------------
# 8. failure is per trajectory
# ---------------------------------------------------------------------------
def test_a_nan_time_step_fails_its_own_slot_only(ilqg):
    c = FdCase(ilqg, "carparking", 0, count=2)
    good, bad = c.solvers
    table, mine = rows("carparking", c.params, names=("h", "limA"))
    broken = {n: a.copy() for n, a in mine.items()}
    broken["h"][64] = np.nan
    out = []
    for q, p in ((good, mine), (bad, broken)):
        q.set_params_batch(p)
        q.init(c.x0, c.u0)
        status_at_init = q.ints("status").copy()
        q.iterate(3)
        out.append((status_at_init, full_state(q)))
    (st_good, a), (st_bad, b) = out
    assert st_bad[64] == 7 and np.all(np.delete(st_bad, 64) == 0) and np.all(st_good == 0)
    keep = np.arange(B) != 64
    states_equal(b, a, "every other slot beside the NaN row", keep, keep)
    c.close()


# ---------------------------------------------------------------------------
# 9. refusals: the error text, an untouched batch, no launch
# ---------------------------------------------------------------------------
def refused(ilqg, s, call, words):
    before, n = full_state(s), None
    s.timing(True)
    n = launches(s)
    with pytest.raises(ilqg.IlqgError) as e:
        call()
    assert all(w in str(e.value) for w in words), str(e.value)
    assert launches(s) == n, "a refused call launched a kernel"
    states_equal(full_state(s), before, "a refused call changed the batch")


def raw(s, entry, names, values, *more):
    import ctypes as C
    arr = None if names is None else (C.c_char_p * max(len(names), 1))(*[n.encode() for n in names])
    ptr = None if values is None else values.ctypes.data_as(C.c_void_p)
    return lambda n_names: s._ck(getattr(s.lib, entry)(s.h, n_names, arr, ptr, *more))


def test_refusals_leave_the_batch_untouched(ilqg, torch):
    import ctypes as C
    for name, fd in (("carparking", 0), ("almix", 1)):
        c = FdCase(ilqg, name, fd, count=2)
        s, never = c.solvers
        table, mine = rows(name, c.params)
        s.set_params_batch(mine)
        for q in (s, never):
            q.init(c.x0, c.u0)
            q.iterate(2)
        first = NAMED[name][0]
        v = np.zeros((B, 8))
        host = "ilqg_batch_set_params_batch"
        refused(ilqg, s, lambda: raw(s, host, ["nope"], v)(1), ("names[0]", "Parameter name 'nope' is not member of parameters struct."))
        refused(ilqg, s, lambda: raw(s, host, [first, first], v)(2), ("names[1]", first, "twice"))
        refused(ilqg, s, lambda: raw(s, host, [first], v)(-1), ("n_names = -1",))
        refused(ilqg, s, lambda: raw(s, host, None, v)(1), ("names is NULL",))
        refused(ilqg, s, lambda: raw(s, host, [first], None)(1), ("values is NULL",))
        if name in PER_STEP:
            refused(ilqg, s, lambda: raw(s, host, [PER_STEP[name]], v)(1), ("names[0]", PER_STEP[name], "one value per time step"))
        refused(ilqg, s, lambda: raw(s, host + "_device", [first], v, None)(1), ("values", "device"))  # host memory in the device form
        refused(ilqg, s, lambda: s.set_param(first, c.params[first]), (first, "per trajectory", "ilqg_batch_set_params_batch(c, 0, NULL, NULL)"))
        refused(ilqg, s, lambda: s.solve_stream(c.x0, c.u0), ("ilqg_batch_solve_stream", "per-trajectory", "table per start"))
        # every refusal left the set as it was: the batch goes on as one that was never disturbed
        other = FdCase(ilqg, name, fd)
        (t,) = other.solvers
        t.set_params_batch(mine)
        t.init(c.x0, c.u0)
        t.iterate(2)
        for q in (s, t):
            q.iterate(3)
        states_equal(full_state(s), full_state(t), "after the refusals")
        # ... and on a batch without a set they leave it without one (test 5: the parent's kernels)
        refused(ilqg, never, lambda: raw(never, host, ["nope"], v)(1), ("nope",))
        refused(ilqg, never, lambda: raw(never, host, [first], v)(-1), ("n_names = -1",))
        plain = FdCase(ilqg, name, fd)
        (p,) = plain.solvers
        p.init(c.x0, c.u0)
        p.iterate(2)
        for q in (never, p):
            q.iterate(3)
        states_equal(full_state(never), full_state(p), "a batch without a set after refusals")
        for q in (c, other, plain):
            q.close()


@pytest.mark.parametrize("name,fd,strict,batch", [("carparking_wave", 0, "wave", B), ("synth16x8", 1, False, 8)])
def test_the_wave_mapping_refuses_and_names_itself(ilqg, name, fd, strict, batch):
    import test_gpu_receding as base
    prob, _, _, N, params, opts, x0, u0 = base.setup(name, batch)
    s = ilqg.BatchSolver(prob, fd, batch=batch, n_hor=N, params=params, opts=dict(opts, max_iter=40), strict=strict)
    s.init(x0, u0)
    s.iterate(1)
    n = NAMED[name][0]
    refused(ilqg, s, lambda: s.set_params_batch({n: np.broadcast_to(np.asarray(params[n], dtype=np.float64), (batch, np.size(params[n])))}),
            ("ilqg_batch_set_params_batch", "wave mapping", "one wavefront"))
    s.close()
