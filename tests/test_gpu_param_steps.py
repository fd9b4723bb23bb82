"""BatchSolver.set_param_steps_batch / param_steps_batch / shift_param_batch on the GPU: every trajectory of a batch plans under
a window of its own of a per-time-step parameter (the rows twins of k_rollout, k_derivs_rows, k_backward, k_search,
k_multipliers_rows and k_policy with a per-lane pointer; k_shift_param_rows; k_move_rows).

Cases are those of tests/param_steps_cases.py (B = 70, SLOTS 0, 63, 64, 69; row[b][k] = nominal[k] (1 + 0.05 N(0, 1)); almix's
`vref` and brachi_hli's `ymin`), which tests/test_param_steps_recipe.py shows to be no no-op on the CPU.  Test 1 and test 8
hold the product against the oracle driver under THAT slot's parameter dict with the tree's single-pass bar
|d| <= 1e-10 max(1, |ref|); every other test is an identity between calls of the product and is bit for bit."""
import ctypes as C

import numpy as np
import pytest

from oracle.harness import almix_case, lib_path
from param_steps_cases import BUILDS, SLOTS, STEP_NAME, B, StepCase, dict_of, oracle_stages, setup, step_rows
from params_batch_cases import rows as fixed_rows
from policy_cases import perturbed_starts, reference_rollout
from policy_param_cases import draws, params_of
from test_gpu_params_batch import close_inf, launches, refused, states_equal
from test_gpu_policy_rollout import close, ilqg, torch, worst  # noqa: F401 (fixtures)
from test_gpu_receding_plant import full_state

pytestmark = pytest.mark.gpu

_ORACLE = {}


def oracle(c, b):
    """the oracle's stages for slot b under its own window, computed once per (problem, FULL_DDP, slot) and shared"""
    key = (c.name, c.fd, b)
    if key not in _ORACLE:
        _ORACLE[key] = oracle_stages(lib_path("oracle", c.name, c.fd), c.N, dict_of(c.name, c.params, c.rows, b), c.opts, c.x0[b], c.u0[b])
    return _ORACLE[key]


# ---------------------------------------------------------------------------
# 1. stage by stage against the reference
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("name,fd,strict", BUILDS)
def test_every_stage_equals_the_oracle_under_the_slots_own_window(ilqg, name, fd, strict):
    c = StepCase(ilqg, name, fd, strict, count=2, opts=dict(ls_split=0))  # (ls_split = 0: every step size is rolled out for every slot)
    s, fused = c.solvers
    dev = {}

    def hold(key, got, want, b):
        dev[key] = max(dev.get(key, 0.0), worst(np.asarray(got)[np.isfinite(want)], np.asarray(want)[np.isfinite(want)]))
        assert close_inf(got, want), "%s fd%d slot %d: %s off by %.3g" % (name, fd, b, key, dev[key])

    for q in (s, fused):
        q.set_param_steps_batch(c.step, c.rows)
        q.init(c.x0, c.u0)
    x, cost = s.x(), s.scalar("cost")
    for b in SLOTS:
        ref = oracle(c, b)
        assert ref["init"] == 1 and s.ints("status")[b] == 0
        hold("x", x[b], ref["x"], b)
        hold("cost", cost[b], ref["cost"], b)
    s.calc_derivs()
    rec, fin = s.derivs()
    nd = s.problem.rec_dev
    for b in SLOTS:
        ref = oracle(c, b)
        hold("records", rec[b][:, :nd], ref["rec"][:, :nd], b)
        hold("final record", fin[b], ref["fin"], b)
    s.back_pass(single_sweep=True)
    fused.back_pass(fused=True)
    for tag, q in (("", s), ("fused ", fused)):
        l, L = q.gains()
        dV0, dV1, rc = q.scalar("dV0"), q.scalar("dV1"), q.ints("bp_rc")
        for b in SLOTS:
            ref = oracle(c, b)
            assert rc[b] == ref["bp_rc"] == 0
            hold(tag + "l", l[b], ref["l"], b)
            hold(tag + "L", L[b], ref["L"], b)
            hold(tag + "dV", [dV0[b], dV1[b]], [ref["dV0"], ref["dV1"]], b)
    s.line_search()
    ac, ok, idx, acc = s.scalar("alpha_cost"), s.ints("alpha_ok"), s.ints("alpha_idx"), s.ints("accepted")
    for b in SLOTS:
        ref = oracle(c, b)
        na = len(ref["alpha_cost"])
        assert np.array_equal(ok[b][:na], ref["alpha_ok"]) and acc[b] == ref["accept"] and idx[b] == ref["alpha_idx"], (name, fd, b)
        hold("alpha_cost", ac[b][:na], ref["alpha_cost"], b)
    print("%s fd%d%s: worst deviation from the oracle under the slots' own windows: " % (name, fd, " FMA-free" if strict else "") +
          ", ".join("%s %.3g" % kv for kv in dev.items()))
    c.close()


# ---------------------------------------------------------------------------
# 2. a batch is its trajectories
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("with_table", [False, True])
def test_a_batch_is_its_trajectories(ilqg, with_table):
    """FMA-free almix, iterate(5) (multiplier updates included): slot b has the bits of a batch of ONE trajectory whose shared
    `vref` (set_param) is row b — and the same with a fixed-size per-trajectory table (tgt, lim) set beside the rows"""
    c = StepCase(ilqg, "almix", 1, True)
    (s,) = c.solvers
    s.set_param_steps_batch("vref", c.rows)
    mine = {}
    if with_table:
        _, mine = fixed_rows("almix", c.params)
        s.set_params_batch(mine)
    s.init(c.x0, c.u0)
    s.iterate(5)
    whole = full_state(s)
    assert np.any(whole["mul_running"] != 0.0)
    for b in SLOTS:
        one = ilqg.BatchSolver("almix", 1, batch=1, n_hor=c.N, params=c.params, opts=dict(c.opts, max_iter=40), strict=True)
        one.set_param("vref", c.rows[b])
        for n, a in mine.items():
            one.set_param(n, a[b])
        one.init(c.x0[b:b + 1], c.u0[b:b + 1])
        one.iterate(5)
        states_equal(full_state(one), whole, "slot %d against a batch of one under set_param" % b, slice(0, 1), slice(b, b + 1))
        one.close()
    c.close()


# ---------------------------------------------------------------------------
# 3. nominal rows, and a cleared name
# ---------------------------------------------------------------------------
def test_nominal_rows_give_the_shared_batch(ilqg):
    c = StepCase(ilqg, "almix", 1, True, count=2)
    shared, per = c.solvers
    nominal = np.asarray(c.params["vref"], dtype=np.float64)
    per.set_param_steps_batch("vref", np.tile(nominal, (B, 1)))
    for q in (shared, per):
        q.init(c.x0, c.u0)
        q.iterate(5)
    states_equal(full_state(per), full_state(shared), "nominal rows against the shared batch")
    assert np.array_equal(per.param_steps_batch("vref"), shared.param_steps_batch("vref"))
    assert np.array_equal(shared.param_steps_batch("vref")[B - 1], nominal)
    c.close()


@pytest.mark.parametrize("name,fd", [("almix", 1), ("brachi_hli", 0)])
def test_a_cleared_name_is_the_batch_that_never_had_rows(ilqg, name, fd):
    """product build, where the rows twins are other code than the kernels without a pack (other contractions): bit for bit
    the batch that never had rows, and the same launches by kernel name"""
    c = StepCase(ilqg, name, fd, count=2)
    never, cleared = c.solvers
    cleared.set_param_steps_batch(c.step, c.rows)
    cleared.init(c.x0, c.u0)
    cleared.iterate(2)
    cleared.set_param_steps_batch(c.step, None)
    assert np.array_equal(cleared.param_steps_batch(c.step), np.tile(np.asarray(c.params[c.step], dtype=np.float64), (B, 1)))
    counts = []
    for q in (never, cleared):
        q.timing(True)
        before = launches(q)
        q.init(c.x0, c.u0)
        q.iterate(5)
        after = launches(q)
        counts.append({k: after[k] - before[k] for k in after})
    assert counts[0] == counts[1], counts
    states_equal(full_state(cleared), full_state(never), "set, iterate, clear, init against a batch without rows")
    cleared.set_param(c.step, c.params[c.step])  # (shared again: set_param of that name is no longer refused)
    cleared.shift_param(c.step, 1)
    c.close()


# ---------------------------------------------------------------------------
# 4. the window shift
# ---------------------------------------------------------------------------
def test_shift_param_batch_equals_the_resent_rows(ilqg):
    """brachi_hli at n_hor = 600: rows of 601 values span three blocks of k_shift_param_rows; no solve is needed"""
    n = 600
    c = StepCase(ilqg, "brachi_hli", 0, count=2, n=n)
    a, b = c.solvers
    rng = np.random.default_rng(7)
    for s in (1, 255, 256, 257, 600):
        tail = rng.standard_normal((B, s))
        for q in (a, b):
            q.set_param_steps_batch("ymin", c.rows)
        a.shift_param_batch("ymin", s, tail)
        moved = np.concatenate([c.rows[:, s:], tail], axis=1)
        b.set_param_steps_batch("ymin", moved)
        assert np.array_equal(a.param_steps_batch("ymin"), moved), s
        assert np.array_equal(a.param_steps_batch("ymin"), b.param_steps_batch("ymin")), s
        a.set_param_steps_batch("ymin", c.rows)
        a.shift_param_batch("ymin", s)  # NULL tail: p[b][n_hor] held
        assert np.array_equal(a.param_steps_batch("ymin"), np.concatenate([c.rows[:, s:], np.repeat(c.rows[:, -1:], s, axis=1)], axis=1)), s
    a.set_param_steps_batch("ymin", c.rows)
    a.shift_param_batch("ymin", 0, None)
    a.shift_param_batch("ymin", 0, np.zeros((B, 0)))
    assert np.array_equal(a.param_steps_batch("ymin"), c.rows)
    c.close()


def test_a_shifted_window_plans_like_the_resent_one(ilqg):
    """almix at n_hor = 64: shift_param_batch, shift(s), iterate(2) against the same with the rows re-sent"""
    n, s = 64, 5
    params, opts, x0, u0 = almix_case(batch=B)
    params = dict(params, vref=np.asarray(params["vref"])[:n + 1])
    u0 = np.ascontiguousarray(u0[:, :n])
    rows = step_rows("almix", params)
    tail = np.random.default_rng(9).uniform(0.5, 1.2, (B, s))
    out = []
    for resend in (False, True):
        q = ilqg.BatchSolver("almix", 1, batch=B, n_hor=n, params=params, opts=dict(opts, max_iter=40))
        q.set_param_steps_batch("vref", rows)
        q.init(x0, u0)
        q.iterate(3)
        if resend:
            q.set_param_steps_batch("vref", np.concatenate([rows[:, s:], tail], axis=1))
        else:
            q.shift_param_batch("vref", s, tail)
        q.shift(s)
        q.iterate(2)
        out.append(full_state(q))
        q.close()
    states_equal(out[0], out[1], "the window moved in place against the rows re-sent")


# ---------------------------------------------------------------------------
# 5. host and device forms
# ---------------------------------------------------------------------------
def test_host_and_device_forms_give_the_same_bits(ilqg, torch):
    s = 4
    c = StepCase(ilqg, "almix", 1, count=2)
    host, dev = c.solvers
    tail = np.random.default_rng(11).uniform(0.5, 1.2, (B, s))
    host.set_param_steps_batch("vref", c.rows)
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):  # the caller's stream: the tensors are made on it, and the library orders itself behind it
        t_rows = torch.tensor(c.rows, dtype=torch.float64, device="cuda:0")
        t_tail = torch.tensor(tail, dtype=torch.float64, device="cuda:0")
        dev.set_param_steps_batch("vref", t_rows, device=True)
    for q in (host, dev):
        q.init(c.x0, c.u0)
        q.iterate(3)
    states_equal(full_state(dev), full_state(host), "device setter against host setter")
    host.shift_param_batch("vref", s, tail)
    with torch.cuda.stream(side):
        dev.shift_param_batch("vref", s, t_tail, device=True)
        dev.shift_param_batch("vref", 2, None, device=True)
    host.shift_param_batch("vref", 2)
    assert np.array_equal(dev.param_steps_batch("vref"), host.param_steps_batch("vref"))
    for q in (host, dev):
        q.shift(s + 2)
        q.iterate(2)
    states_equal(full_state(dev), full_state(host), "device shift against host shift")
    side.synchronize()
    c.close()


# ---------------------------------------------------------------------------
# 6. identities
# ---------------------------------------------------------------------------
def run(s, c, rows, flip=False):
    s.set_param_steps_batch(c.step, rows)
    s.init(c.x0[::-1].copy() if flip else c.x0, c.u0[::-1].copy() if flip else c.u0)
    s.iterate(6)
    return full_state(s)


def test_groups_and_shards_hold_their_slices_of_the_rows(ilqg):
    """B = 200 is four stream groups of 64 (the last one ragged): groups 1 against 4, and two loop-back shards of a
    MultiSolver, each with the rows (and tails) from its first trajectory on"""
    n, sh = 200, 3
    cases = [StepCase(ilqg, "almix", 1, groups=g, batch=n) for g in (1, 4)]
    c = cases[0]
    tail = np.random.default_rng(13).uniform(0.5, 1.2, (n, sh))
    outs = []
    for q in cases:
        (s,) = q.solvers
        run(s, q, c.rows)
        s.shift_param_batch("vref", sh, tail)
        s.shift(sh)
        s.iterate(2)
        outs.append((full_state(s), s.param_steps_batch("vref")))
    states_equal(outs[1][0], outs[0][0], "four stream groups against one")
    assert np.array_equal(outs[1][1], outs[0][1]) and np.array_equal(outs[0][1], np.concatenate([c.rows[:, sh:], tail], axis=1))
    m = ilqg.MultiSolver("almix", 1, batch=n, n_hor=c.N, devices=[0, 0], params=c.params, opts=dict(c.opts, max_iter=40))
    m.set_param_steps_batch("vref", c.rows)
    m.init(c.x0, c.u0)
    m.iterate(6)
    m.shift_param_batch("vref", sh, tail)
    m.shift(sh)
    m.iterate(2)
    base = outs[0][0]
    assert np.array_equal(m.x(), base["x"]) and np.array_equal(m.u(), base["u"])
    assert np.array_equal(m.ints("iterations"), base["iterations"]) and np.array_equal(m.ints("status"), base["status"])
    m.close()
    for q in cases:
        q.close()


@pytest.mark.parametrize("name,fd", [("almix", 1), ("brachi_hli", 1)])
def test_reversed_batch_and_set_clear_set(ilqg, name, fd):
    c = StepCase(ilqg, name, fd, count=3)
    base = run(c.solvers[0], c, c.rows)
    got = run(c.solvers[1], c, c.rows[::-1].copy(), flip=True)
    states_equal({k: v[::-1] for k, v in got.items()}, base, "the reversed batch with reversed rows")
    s = c.solvers[2]
    s.set_param_steps_batch(c.step, c.rows[::-1].copy())
    s.set_param_steps_batch(c.step, None)
    states_equal(run(s, c, c.rows), base, "set, clear, set again")
    c.close()


# ---------------------------------------------------------------------------
# 7. compaction: the rows travel with their trajectories
# ---------------------------------------------------------------------------
def test_a_compacted_solve_equals_the_plain_one(ilqg):
    """almix FULL_DDP 1, B = 300, the case's max_iter = 80, compact = 16 (the recipe test: the rows imply a gather)"""
    n = 300
    N, params, opts, x0, u0 = setup("almix", n)
    rows = step_rows("almix", params, n)
    out = []
    for compact in (0, 16):
        s = ilqg.BatchSolver("almix", 1, batch=n, n_hor=N, params=params, opts=dict(opts, compact=compact))
        s.set_param_steps_batch("vref", rows)
        s.init(x0, u0)
        s.solve()
        o = full_state(s)
        o["trace"] = s.solve_trace()
        for k in ("lambda", "dlambda", "g_norm", "dV0", "dV1", "new_cost", "dcost", "expected", "alpha_cost"):
            o[k] = s.scalar(k).copy()
        for k in ("alpha_idx", "accepted", "bp_calls", "alpha_ok"):
            o[k] = s.ints(k).copy()
        assert np.array_equal(s.param_steps_batch("vref"), rows)  # (the caller's batch keeps its rows)
        out.append(o)
        s.close()
    plain, comp = out
    assert comp["trace"][3] >= 1 and plain["trace"][3] == 0, comp["trace"]
    for k in plain:
        if k != "trace":
            assert np.array_equal(plain[k], comp[k]), k


# ---------------------------------------------------------------------------
# 8. roll-outs of the policy inherit the trajectory's window
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("name,fd", [("almix", 1), ("brachi_hli", 0)])
def test_policy_rollouts_run_under_the_trajectorys_window(ilqg, name, fd):
    R = 5
    c = StepCase(ilqg, name, fd)
    (s,) = c.solvers
    s.set_param_steps_batch(c.step, c.rows)
    s.init(c.x0, c.u0)
    s.iterate(4)
    # (brachi_hli: every roll-out from the case's one start, y = -eps, where the reference's own forward_pass is not finite from
    # any other — the roll-outs then differ through the trajectory's window and, below, the roll-out's own parameters)
    starts = perturbed_starts(c.x0, R, seed=17, sigma=0.1 if name == "almix" else 0.0)
    plain = s.policy_rollout(starts, 1.0, True, trajectories=True)
    # fixed-size names per roll-out on top: the per-step row stays the trajectory's
    fixed = ("tgt", "lim") if name == "almix" else ("g",)
    roll = draws(c.params, fixed, B, R, seed=71)
    named = s.policy_rollout(starts, 1.0, True, trajectories=True, params=roll)
    h = s.head(c.N, gains=True)
    cost = s.scalar("cost")
    w_l, w_f = s.scalar("w_pen_l"), s.scalar("w_pen_f")
    m_run, m_fin = s.multipliers()
    lib = lib_path("oracle", name, fd)
    dev = 0.0
    for b in SLOTS:
        policy = (h["x"][b], h["u"][b], h["l"][b], h["L"][b])
        kw = dict(cost=cost[b], w_pen=(w_l[b], w_f[b]), multipliers=(m_run[b], m_fin[b]))
        mine = dict_of(name, c.params, c.rows, b)
        for r in range(R):
            for out, p in ((plain, mine), (named, params_of(mine, roll, b, r))):
                ok, cr, xr, ur = reference_rollout(lib, c.N, p, c.opts, starts[b, r], policy, 1.0, 1, **kw)
                assert ok == 1 and out["ok"][b, r] == 1, (b, r)
                for got, want in ((out["cost"][b, r], cr), (out["x"][b, r], xr), (out["u"][b, r], ur), (out["x_end"][b, r], xr[-1])):
                    dev = max(dev, worst(got, want))
                    assert close(got, want), "%s slot %d start %d: off by %.3g" % (name, b, r, worst(got, want))
    print("%s: policy roll-outs under the trajectories' windows, worst deviation from the oracle %.3g" % (name, dev))
    c.close()


# ---------------------------------------------------------------------------
# 9. failure is per trajectory
# ---------------------------------------------------------------------------
def test_a_nan_in_one_row_fails_its_own_slot_only(ilqg):
    c = StepCase(ilqg, "almix", 1, count=2)
    good, bad = c.solvers
    broken = c.rows.copy()
    broken[64, 17] = np.nan
    out = []
    for q, rows in ((good, c.rows), (bad, broken)):
        q.set_param_steps_batch("vref", rows)
        q.init(c.x0, c.u0)
        status_at_init = q.ints("status").copy()
        q.iterate(3)
        roll = q.policy_rollout(c.x0[:, None], 0.0, False)
        out.append((status_at_init, full_state(q), roll))
    (st_good, a, roll_good), (st_bad, b, roll_bad) = out
    print("status at init of the slot with the NaN: %d" % st_bad[64])
    assert st_bad[64] != 0 and np.all(np.delete(st_bad, 64) == 0) and np.all(st_good == 0)
    keep = np.arange(B) != 64
    states_equal(b, a, "every other slot beside the NaN row", keep, keep)
    assert roll_bad["ok"][64, 0] == 0 and np.all(roll_bad["ok"][keep] == 1) and np.all(roll_good["ok"] == 1)
    assert np.array_equal(roll_bad["cost"][keep], roll_good["cost"][keep])
    c.close()


# ---------------------------------------------------------------------------
# 10. refusals: the error text, an untouched batch, no launch
# ---------------------------------------------------------------------------
def ptr(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def test_refusals_leave_the_batch_untouched(ilqg, torch):
    c = StepCase(ilqg, "almix", 1, count=2)
    s, t = c.solvers
    for q in (s, t):
        q.set_param_steps_batch("vref", c.rows)
        q.init(c.x0, c.u0)
        q.iterate(2)
    lib, h, N = s.lib, s.h, c.N
    v, tail = np.zeros((B, N + 1)), np.zeros((B, N + 1))
    nominal = np.asarray(c.params["vref"], dtype=np.float64)
    for entry, args in (("ilqg_batch_set_param_steps_batch", (ptr(v),)), ("ilqg_batch_get_param_steps_batch", (ptr(v),)),
                        ("ilqg_batch_shift_param_batch", (1, ptr(tail)))):
        call = getattr(lib, entry)
        refused(ilqg, s, lambda: s._ck(call(h, b"nope", *args)), (entry, "name", "Parameter name 'nope' is not member of parameters struct."))
        refused(ilqg, s, lambda: s._ck(call(h, b"tgt", *args)), (entry, "name", "tgt", "fixed size of 3", "ilqg_batch_set_params_batch"))
        assert call(None, b"vref", *args) != 0  # c NULL
    refused(ilqg, s, lambda: s._ck(lib.ilqg_batch_get_param_steps_batch(h, b"vref", None)), ("ilqg_batch_get_param_steps_batch", "out is NULL"))
    for steps in (-1, N + 1):
        refused(ilqg, s, lambda: s.shift_param_batch("vref", steps), ("ilqg_batch_shift_param_batch", "steps = %d" % steps, "n_hor = %d" % N))
    # host memory in the device forms
    refused(ilqg, s, lambda: s._ck(lib.ilqg_batch_set_param_steps_batch_device(h, b"vref", ptr(v), None)), ("values", "device"))
    refused(ilqg, s, lambda: s._ck(lib.ilqg_batch_shift_param_batch_device(h, b"vref", 2, ptr(tail), None)), ("tail", "device"))
    # the shared forms of a name that has rows
    refused(ilqg, s, lambda: s.set_param("vref", nominal), ("ilqg_batch_set_param", "vref", "per trajectory", "ilqg_batch_shift_param_batch", "values = NULL"))
    refused(ilqg, s, lambda: s.shift_param("vref", 1), ("ilqg_batch_shift_param", "vref", "per trajectory", "ilqg_batch_shift_param_batch", "values = NULL"))
    refused(ilqg, s, lambda: s.solve_stream(c.x0, c.u0), ("ilqg_batch_solve_stream", "per-trajectory", "rows per start"))
    # a per-time-step name stays refused where it was
    refused(ilqg, s, lambda: s._ck(lib.ilqg_batch_set_params_batch(h, 1, (C.c_char_p * 1)(b"vref"), ptr(v))), ("names[0]", "vref", "one value per time step"))
    refused(ilqg, s, lambda: s.receding(1, 1, 1), ())
    assert np.array_equal(s.param_steps_batch("vref"), c.rows)
    # every refusal left the rows as they were: the batch goes on as one that was never disturbed
    for q in (s, t):
        q.iterate(3)
    states_equal(full_state(s), full_state(t), "after the refusals")
    # the window shift of a name that is shared (the getter is allowed there)
    s.set_param_steps_batch("vref", None)
    assert np.array_equal(s.param_steps_batch("vref"), np.tile(nominal, (B, 1)))
    refused(ilqg, s, lambda: s.shift_param_batch("vref", 1), ("ilqg_batch_shift_param_batch", "vref", "currently shared", "ilqg_batch_set_param_steps_batch"))
    c.close()


def test_the_wave_mapping_refuses_and_names_itself(ilqg):
    c = StepCase(ilqg, "brachi_hli", 0, "wave", batch=8)
    (s,) = c.solvers
    s.init(c.x0, c.u0)
    s.iterate(1)
    for call, entry in ((lambda: s.set_param_steps_batch("ymin", c.rows), "ilqg_batch_set_param_steps_batch"),
                        (lambda: s.shift_param_batch("ymin", 1), "ilqg_batch_shift_param_batch"),
                        (lambda: s.param_steps_batch("ymin"), "ilqg_batch_get_param_steps_batch")):
        refused(ilqg, s, call, (entry, "wave mapping", "one wavefront"))
    c.close()
