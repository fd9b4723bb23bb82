"""BatchSolver.receding_plant on the GPU: the closed loop of planner and plant (ilqg_batch_receding_plant, k_plant).

Per round: iterate(2); every trajectory's plant advances `steps` steps from its own state under the plan's policy
(u = u_nom_k [+ L_k (x_plant - x_nom_k)]), each step the reference's forward_pass step (iLQG_func.tem:121-185) under the
PLANT's parameters, the disturbance added behind it; then shift(steps, x0 = the plants' states).

Tests 1, 7, 8 and 9 hold the logs against the reference's own forward_pass through the CPU oracle's driver under each compared
trajectory's parameter dict (tests/policy_cases.py, tests/policy_param_cases.py, tests/plant_cases.py) with the tree's
single-pass bar, |d| <= 1e-10 max(1, |ref|).  Tests 2 and 4 hold the loop against compositions of entries that existed before
(bit for bit in the FMA-free builds), test 3 holds identities within the new code bit for bit, tests 5 and 6 failures and
refusals.  Builds, inputs, B = 70 (one full and one partly filled wavefront), SLOTS and Case are those of
tests/test_gpu_policy_rollout.py; rounds = 3 and iterations = 2 unless a test says otherwise.

The sum of the applied running costs (`cost`) is held against the reference too: forward_pass leaves every step's cost in the
candidate trajectory, and the oracle's driver returns them (Driver.step_costs).  Test 1 compares `cost` with the sum of the
first `steps` of them, in step order from 0.0 under the plant's parameters; tests 7 to 9 with policy_cases.reference_plant, the
chain of one-step roll-outs that also takes a disturbance inside a round (the read of the table at the steps before the last
one, x_next + w, and the feedback of the next step from the disturbed state) and, teacher-forced on the device's own plant
states, the later rounds.  tests/test_plant_reference_recipe.py pins that chain to the reference build without a GPU and shows
that the cost under the model's parameters, a dropped inner disturbance and the wrong order of two overrides each miss the bar
by 1e4 times or more.  The identities of tests 3 and 5 hold `cost` as before."""
import ctypes as C

import numpy as np
import pytest

from oracle.harness import lib_path
from plant_cases import SHORT_N, SHORT_SEED, noise, plant_rows, plant_starts, short_car  # noqa: F401
from policy_cases import reference_plant, reference_rollout
from policy_param_cases import NAMED, PER_STEP, SCALE, draws, nominal_table, params_of
from test_gpu_policy_rollout import B, SLOTS, Case, assert_state_equal, close, ilqg, outputs_equal, state, worst  # noqa: F401

pytestmark = pytest.mark.gpu

ROUNDS, ITERATIONS = 3, 2
LOGS = ("x", "u", "cost", "plan_cost", "ok", "x_plant")


def full_state(s):
    """what the issue's bit-for-bit comparison of a batch names: x, u, gains, cost, status, iterations, lambda (and the
    multipliers and penalty weights of a problem that has them)"""
    out = state(s)
    out["l"], out["L"] = s.gains()
    return out


def plan_of(b):
    """slot -> (policy, what reference_rollout / reference_plant take beside it) of the batch's current plans: heads with
    gains, costs, and the multipliers and penalty weights of a problem that has them"""
    h = b.head(b.N, gains=True)
    cost = b.scalar("cost")
    mul = sum(b.multiplier_dims()) > 0
    w_l, w_f = (b.scalar("w_pen_l"), b.scalar("w_pen_f")) if mul else (np.zeros(b.B), np.zeros(b.B))
    m_run, m_fin = b.multipliers() if mul else (None, None)
    return lambda s: ((h["x"][s], h["u"][s], h["l"][s], h["L"][s]),
                      dict(cost=cost[s], w_pen=(w_l[s], w_f[s]), multipliers=(m_run[s], m_fin[s]) if mul else None))


def hold_rounds(c, out, twin, plant, X, w, rounds, steps, feedback, what, iterations=ITERATIONS):
    """the logs `out` of receding_plant(rounds, steps, iterations, feedback, X, ..., w) against policy_cases.reference_plant,
    round by round, teacher-forced on the device's own plant states: the twin batch (the loop's inputs) runs iterate, its
    plans' policies are read, the reference's plant goes from X_r = out["x"][:, r * steps] (round 0: the given X) under
    plant(s), slot s's parameter dict, and that round's slice of w, and the twin is shifted to X_{r+1} (behind the last round
    out["x_plant"]).  plan_cost: the twin's, bit for bit (the same kernels on the same bits).  x, u, cost[:, r] and
    X_{r+1} against the reference's at the single-pass bar.  Returns the worst deviations."""
    lib = lib_path("oracle", c.problem, c.fd)
    dev = dict(x=0.0, u=0.0, cost=0.0, x_plant=0.0)
    assert np.all(out["ok"] == 1), what
    Xr = X
    for r in range(rounds):
        twin.iterate(iterations)
        plan = plan_of(twin)
        assert np.array_equal(out["plan_cost"][:, r], twin.scalar("cost")), "%s round %d: the plans' costs are not the twin's" % (what, r)
        lo, hi = r * steps, (r + 1) * steps
        nxt = out["x"][:, hi] if r + 1 < rounds else out["x_plant"]
        for s in SLOTS:
            policy, kw = plan(s)
            x, u, _, cost, x_end = reference_plant(lib, c.N, plant(s), c.opts, Xr[s], policy, feedback, steps, w=w[s, lo:hi], **kw)
            assert all(np.all(np.isfinite(v)) for v in (x, u, cost, x_end)), "%s round %d slot %d: the reference is not finite (a compared slot may not be left out)" % (what, r, s)
            got = dict(x=out["x"][s, lo:hi], u=out["u"][s, lo:hi], cost=out["cost"][s, r], x_plant=nxt[s])
            want = dict(x=x, u=u, cost=cost, x_plant=x_end)
            for k in got:
                dev[k] = max(dev[k], worst(got[k], want[k]))
            for k in got:
                assert close(got[k], want[k]), "%s round %d slot %d: %s off by %.3g" % (what, r, s, k, worst(got[k], want[k]))
        twin.shift(steps, x0=np.ascontiguousarray(nxt))
        Xr = nxt
    return dev


def composition(b, rows, X, w, rounds, steps, iterations=ITERATIONS):
    """rounds x { iterate; policy_rollout(x_plant[:, None], alpha = 0, feedback, trajectories, params = rows[:, None]); x, u of
    the first `steps` steps; x_plant = x[steps] + w of the round's LAST step (policy_rollout has no disturbance inside a
    roll-out); shift(steps, x0 = x_plant) } on batch b: what the loop's x, u, plan_cost and x_plant are compared with"""
    xp, xs, us, pc = X.copy(), [], [], []
    for r in range(rounds):
        b.iterate(iterations)
        pc.append(b.scalar("cost"))
        o = b.policy_rollout(xp[:, None], alpha=0.0, feedback=True, trajectories=True, params={n: t[:, None] for n, t in rows.items()})
        assert np.all(o["ok"] == 1)
        xs.append(o["x"][:, 0, 0:steps]), us.append(o["u"][:, 0, 0:steps])
        xp = o["x"][:, 0, steps] + w[:, r * steps + steps - 1]
        b.shift(steps, x0=xp)
    return dict(x=np.concatenate(xs, axis=1), u=np.concatenate(us, axis=1), plan_cost=np.stack(pc, axis=1), x_plant=xp)


class ShortCase(Case):
    """Case for CarParking with the horizon of SHORT_N steps (tests/plant_cases.py short_car)"""

    def __init__(self, ilqg, count=1, strict=False):
        self.name, self.problem, self.fd, self.opts, self.plant_seed = "carparking", "carparking", 0, {}, SHORT_SEED
        self.N, self.params, self.x0, self.u0 = short_car()
        self.solvers = [ilqg.BatchSolver("carparking", 0, batch=B, n_hor=self.N, params=self.params, opts=dict(max_iter=40), strict=strict, groups=0)
                        for _ in range(count)]
        self.nx, self.nu = self.solvers[0].problem.nx, self.solvers[0].problem.nu


# ---------------------------------------------------------------------------
# 1. one round against the reference's forward_pass under the plant's parameters
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("feedback", [1, 0])
@pytest.mark.parametrize("name,strict", [(n, None) for n in NAMED] + [("synth16x8", True)])
def test_one_round_equals_the_references_forward_pass_under_the_plants_parameters(ilqg, name, strict, feedback):
    """rounds = 1, steps = 3, a disturbance on the last step only.  The policy, multipliers and penalty weights are read from
    a twin batch advanced by iterate(2) alone (identical inputs; lock-step iterations are deterministic).  strict=True: the
    FMA-free n = 16 build, which reads the plant's parameters from memory.  almix has a per-time-step parameter: the loop
    refuses it, which is what is asserted for it here.  The applied cost is compared with the sum of the first three step
    costs of the same forward_pass, in step order from 0.0 (the disturbance sits behind the last step: no step's cost reads
    it)."""
    steps = 3
    c = Case(ilqg, name, 0, count=2, strict=strict)
    a, b = c.history("init")
    table, rows = plant_rows(c)
    X, w = plant_starts(c), noise(c, steps, rounds=1, last_only=True)
    if name in PER_STEP:
        with pytest.raises(ilqg.IlqgError) as e:
            a.receding_plant(1, steps, ITERATIONS, bool(feedback), X, rows, w)
        assert "ilqg_batch_receding_plant" in str(e.value) and PER_STEP[name] in str(e.value) and "ilqg_batch_shift" in str(e.value)
        c.close()
        return
    out = a.receding_plant(1, steps, ITERATIONS, bool(feedback), X, rows, w)
    assert out["x"].shape == (B, steps, c.nx) and out["u"].shape == (B, steps, c.nu) and out["cost"].shape == (B, 1) and out["ok"].dtype == np.int32
    b.iterate(ITERATIONS)
    h = b.head(c.N, gains=True)
    cost = b.scalar("cost")
    mul = sum(b.multiplier_dims()) > 0
    w_l, w_f = (b.scalar("w_pen_l"), b.scalar("w_pen_f")) if mul else (np.zeros(B), np.zeros(B))
    m_run, m_fin = b.multipliers() if mul else (None, None)
    assert np.array_equal(out["plan_cost"][:, 0], cost)
    assert np.all(out["ok"] == 1)
    oracle = lib_path("oracle", c.problem, c.fd)
    dev = dict(x=0.0, u=0.0, x_plant=0.0, cost=0.0)
    for s in SLOTS:
        policy = (h["x"][s], h["u"][s], h["l"][s], h["L"][s])
        ok, _, xr, ur, sc = reference_rollout(oracle, c.N, params_of(c.params, table, s, 1), c.opts, X[s], policy, 0.0, feedback, cost=cost[s],
                                              w_pen=(w_l[s], w_f[s]), multipliers=(m_run[s], m_fin[s]) if mul else None, step_costs=True)
        what = "%s strict=%s feedback=%d slot %d" % (name, strict, feedback, s)
        assert ok == 1 and np.all(np.isfinite(xr)) and np.all(np.isfinite(ur)) and np.all(np.isfinite(sc)), what + ": the oracle's roll-out is not finite (a compared slot may not be left out)"
        applied = 0.0
        for k in range(steps):
            applied += sc[k]
        got = dict(x=out["x"][s], u=out["u"][s], x_plant=out["x_plant"][s], cost=out["cost"][s, 0])
        want = dict(x=xr[0:steps], u=ur[0:steps], x_plant=xr[steps] + w[s, steps - 1], cost=applied)
        for k in got:
            dev[k] = max(dev[k], worst(got[k], want[k]))
        for k in got:
            assert close(got[k], want[k]), "%s: %s off by %.3g" % (what, k, worst(got[k], want[k]))
    print("%s strict=%s feedback=%d: worst deviation from the oracle's forward_pass " % (name, strict, feedback) + ", ".join("%s %.3g" % kv for kv in dev.items()))
    c.close()


# ---------------------------------------------------------------------------
# 2. the loop composed from the public entries
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("steps", [1, 4])
@pytest.mark.parametrize("name,strict", [("carparking", True), ("synth16x8", True), ("carparking", None), ("synth16x8", None)])
def test_loop_equals_the_public_composition(ilqg, name, strict, steps):
    """One call against the loop { iterate(2); policy_rollout(x_plant[:, None], alpha = 0, feedback, trajectories, params =
    rows[:, None]); x, u of the first `steps` steps; x_plant = x[steps] + w; shift(steps, x0 = x_plant) }.  steps = 1 with a
    dense disturbance, steps = 4 with one on each round's last step only (policy_rollout has no disturbance inside a
    roll-out).  FMA-free builds, three rounds: the logs, x_plant and the batch's state afterwards bit for bit.  Product builds,
    one round: the 1e-10 bar (k_plant and k_policy<true> are different kernels: other FMA contractions)."""
    rounds = ROUNDS if strict else 1
    c = Case(ilqg, name, 0, count=2, strict=strict)
    a, b = c.history("init")
    _, rows = plant_rows(c)
    X, w = plant_starts(c), noise(c, steps, rounds=rounds, last_only=steps > 1)
    out = a.receding_plant(rounds, steps, ITERATIONS, True, X, rows, w)
    assert np.all(out["ok"] == 1)
    want = composition(b, rows, X, w, rounds, steps)
    print("%s strict=%s steps=%d: worst deviation from the composition " % (name, strict, steps) + ", ".join("%s %.3g" % (k, worst(out[k], v)) for k, v in want.items()))
    if strict:
        outputs_equal(out, want, "one call against the composition, FMA-free build", sorted(want))
        assert_state_equal(full_state(a), full_state(b), "%s: the batch behind the loop" % name)
    else:
        for k, v in want.items():
            assert close(out[k], v), k
    c.close()


# ---------------------------------------------------------------------------
# 3. identities within the new code, bit for bit
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["carparking", "carparking_wave", "synth16x8"])
def test_one_call_of_three_rounds_is_three_calls_of_one(ilqg, name):
    steps = 2
    c = Case(ilqg, name, 0, count=2)
    a, b = c.history("init")
    _, rows = plant_rows(c)
    X, w = plant_starts(c), noise(c, steps)
    one = a.receding_plant(ROUNDS, steps, ITERATIONS, True, X, rows, w)
    xp, parts = X, []
    for r in range(ROUNDS):
        parts.append(b.receding_plant(1, steps, ITERATIONS, True, xp, rows, w[:, r * steps:(r + 1) * steps]))
        xp = parts[-1]["x_plant"]
    joined = {k: np.concatenate([p[k] for p in parts], axis=1) for k in ("x", "u", "cost", "plan_cost")}
    joined.update(ok=np.min([p["ok"] for p in parts], axis=0), x_plant=xp)
    assert np.all(one["ok"] == 1)
    outputs_equal(one, joined, "%s: three rounds against three calls of one" % name, LOGS)
    assert_state_equal(full_state(a), full_state(b), "%s: the batch behind the loop" % name)
    c.close()


def test_groups_shards_name_order_and_an_extra_nominal_parameter_give_the_same_bits(ilqg):
    """B = 200 here: a group is whole tiles of 64 trajectories, so four groups need more than three tiles.  Shards: two
    loop-back shards of MultiSolver on one device (the fixture of tests/test_gpu_policy_rollout_params.py)."""
    n, steps = 200, 2
    cases = [Case(ilqg, "carparking", g, batch=n) for g in (1, 4)]
    c = cases[0]
    names = NAMED["carparking"]
    _, rows = plant_rows(c, batch=n)
    X, w = plant_starts(c), noise(c, steps, batch=n)
    outs = []
    for q in cases:
        (s,) = q.history("init")
        outs.append(s.receding_plant(ROUNDS, steps, ITERATIONS, True, X, rows, w))
    assert np.all(outs[0]["ok"] == 1)
    outputs_equal(outs[1], outs[0], "four stream groups against one", LOGS)
    assert_state_equal(full_state(cases[1].solvers[0]), full_state(cases[0].solvers[0]), "four stream groups against one: the batch")
    m = ilqg.MultiSolver("carparking", 0, batch=n, n_hor=c.N, devices=[0] * 2, params=c.params, opts=dict(max_iter=40))
    m.init(c.x0, c.u0)
    outputs_equal(m.receding_plant(ROUNDS, steps, ITERATIONS, True, X, rows, w), outs[0], "two shards against the single batch", LOGS)
    one = c.solvers[0]
    assert np.array_equal(m.x(), one.x()) and np.array_equal(m.u(), one.u()) and np.array_equal(m.ints("iterations"), one.ints("iterations"))
    m.close()
    # the names in another order, the columns with them; an extra parameter named with the batch's own value
    (s,) = c.history("init")
    outputs_equal(s.receding_plant(ROUNDS, steps, ITERATIONS, True, X, {k: rows[k] for k in reversed(names)}, w), outs[0], "names in reverse order", LOGS)
    extra = next(k for k, size in s.problem.params if size > 0 and k not in names)
    more = dict(rows, **{extra: nominal_table(c.params, (extra,), n, 1)[extra][:, 0]})
    (s,) = c.history("init")
    outputs_equal(s.receding_plant(ROUNDS, steps, ITERATIONS, True, X, more, w), outs[0], "%s named with its nominal value" % extra, LOGS)
    for q in cases:
        q.close()


@pytest.mark.parametrize("name", ["carparking", "synth16x8"])
def test_the_batchs_own_parameters_are_unchanged(ilqg, name):
    """both batches run the same loop; one is then given every parameter anew (which sends the table again).  An initial
    roll-out and two iterations later the two still agree bit for bit: the planner's parameters are the batch's."""
    steps = 2
    c = Case(ilqg, name, 0, count=2)
    a, b = c.history("init")
    _, rows = plant_rows(c)
    X, w = plant_starts(c), noise(c, steps)
    outputs_equal(a.receding_plant(ROUNDS, steps, ITERATIONS, True, X, rows, w), b.receding_plant(ROUNDS, steps, ITERATIONS, True, X, rows, w), "twins", LOGS)
    for k, v in c.params.items():
        b.set_param(k, v)
    for s in (a, b):
        s.shift(0)
        s.iterate(2)
    assert_state_equal(full_state(a), full_state(b), "%s: behind the loop, parameters sent anew against left alone" % name)
    c.close()


# ---------------------------------------------------------------------------
# 4. no plant, no noise, no feedback: the model loop
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("strict", [True, None])
def test_without_plant_noise_and_feedback_the_loop_is_receding(ilqg, strict):
    """n_names = 0, disturbance NULL, feedback = 0, x_plant NULL against ilqg_batch_receding: in the FMA-free CarParking build
    x, u, the plans' costs and the batch afterwards bit for bit (the plant's step has the bits of the roll-out that stored
    the plan); in the product build the first round within the 1e-10 bar."""
    steps = 3
    c = Case(ilqg, "carparking", 0, count=2, strict=strict)
    a, b = c.history("init")
    out = a.receding_plant(ROUNDS, steps, ITERATIONS, feedback=False)
    ref = b.receding(ROUNDS, steps, ITERATIONS)
    assert out["x_plant"] is None and np.all(out["ok"] == 1)
    print("strict=%s: worst deviation from receding x %.3g, u %.3g, plan_cost %.3g" % (strict, worst(out["x"], ref["x"]), worst(out["u"], ref["u"]),
                                                                                  worst(out["plan_cost"], ref["cost"])))
    if strict:
        assert np.array_equal(out["x"], ref["x"]) and np.array_equal(out["u"], ref["u"]) and np.array_equal(out["plan_cost"], ref["cost"])
        assert_state_equal(full_state(a), full_state(b), "the batch behind the loop")
    else:
        assert close(out["x"][:, :steps], ref["x"][:, :steps]) and close(out["u"][:, :steps], ref["u"][:, :steps])
        assert close(out["plan_cost"][:, 0], ref["cost"][:, 0])
    c.close()


# ---------------------------------------------------------------------------
# 5. failure is per trajectory
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["carparking", "synth10hx"])
def test_failure_is_per_trajectory(ilqg, name):
    """the time step h of trajectory 64's plant is NaN — data, not a fault —: ok = 0 for it alone, its plant stays at its
    start, and every other trajectory has the bits of the run without the NaN.  The same for a start with a NaN
    component (trajectory 5)."""
    steps = 2
    c = Case(ilqg, name, 0, count=3)
    a, b, d = c.history("init")
    names = NAMED[name] if "h" in NAMED[name] else NAMED[name] + ("h",)
    rows = {n: np.ascontiguousarray(t[:, 1]) for n, t in draws(c.params, names, B, 2, scale=SCALE[name]).items()}
    X, w = plant_starts(c), noise(c, steps)
    clean = a.receding_plant(ROUNDS, steps, ITERATIONS, True, X, rows, w)
    assert np.all(clean["ok"] == 1)
    bad_rows = {n: t.copy() for n, t in rows.items()}
    bad_rows["h"][64, 0] = np.nan
    bad_X = X.copy()
    bad_X[5, 1] = np.nan
    for s, victim, got in ((b, 64, b.receding_plant(ROUNDS, steps, ITERATIONS, True, X, bad_rows, w)),
                           (d, 5, d.receding_plant(ROUNDS, steps, ITERATIONS, True, bad_X, rows, w))):
        keep = np.ones(B, dtype=bool)
        keep[victim] = False
        assert got["ok"][victim] == 0 and np.all(got["ok"][keep] == 1), victim
        for k in LOGS:
            assert np.array_equal(got[k][keep], clean[k][keep]), "%s: %s of another trajectory changed beside failed trajectory %d" % (name, k, victim)
        assert np.array_equal(got["x_plant"][victim], (X if victim == 64 else bad_X)[victim], equal_nan=True), "the failed plant is not at its start"
        sa, ss = full_state(a), full_state(s)
        for k in sa:
            assert np.array_equal(sa[k][keep], ss[k][keep]), "%s: the batch's %s of another trajectory changed" % (name, k)
    c.close()


# ---------------------------------------------------------------------------
# 6. refusals
# ---------------------------------------------------------------------------
def test_refused_calls_name_the_argument_change_nothing_and_launch_nothing(ilqg):
    steps = 2
    c = Case(ilqg, "carparking", 2, count=2)
    a, b = c.history("mid")
    names = NAMED["carparking"]
    _, rows = plant_rows(c)
    V = np.ascontiguousarray(np.concatenate([rows[n] for n in names], axis=-1))
    X, w = plant_starts(c), noise(c, steps)
    n = ROUNDS * steps
    logs = dict(x=np.full((B, n, c.nx), -7.0), u=np.full((B, n, c.nu), -7.0), cost=np.full((B, ROUNDS), -7.0), plan_cost=np.full((B, ROUNDS), -7.0),
                ok=np.full(B, -7, dtype=np.int32))
    xp = X.copy()

    def strings(*words):
        return (C.c_char_p * max(len(words), 1))(*[v.encode() for v in words])

    def ptr(arr):
        return None if arr is None else C.c_void_p(arr.ctypes.data)

    def raw(rounds=ROUNDS, steps=steps, iterations=ITERATIONS, n_names=len(names), arr=strings(*names), values=V, outputs=True):
        return lambda: a._ck(a.lib.ilqg_batch_receding_plant(a.h, rounds, steps, iterations, 1, ptr(xp), n_names, arr, ptr(values), ptr(w),
                                                             *[ptr(logs[k]) if outputs else None for k in ("x", "u", "cost", "plan_cost", "ok")]))

    def refused(call, *words):
        with pytest.raises(ilqg.IlqgError) as e:
            call()
        for v in ("ilqg_batch_receding_plant",) + words:
            assert v in str(e.value), (v, str(e.value))

    a.timing(True)
    for r in (0, -1):
        refused(raw(rounds=r), "rounds")
    refused(raw(iterations=-1), "iterations")
    for s in (0, -1, c.N, c.N + 5):
        refused(raw(steps=s), "steps", "n_hor")
    refused(raw(n_names=-1), "n_names")
    refused(raw(arr=None), "names")
    refused(raw(values=None), "values")
    refused(raw(arr=strings(*(names[:-1] + ("nope",)))), "names", "Parameter name 'nope' is not member of parameters struct.")
    refused(raw(arr=strings(*(names[:-1] + (names[0],)))), "names", "'%s'" % names[0], "twice")
    assert a.kernel_times()["k_plant"][0] == 0, "a refused call launched the plant"
    assert np.array_equal(xp, X) and all(np.all(v == -7) for v in logs.values()), "a refused call wrote an output"
    assert_state_equal(full_state(a), full_state(b), "the batch behind refused calls")
    # a problem with a per-time-step parameter, and naming it (the same refusal comes first)
    q = Case(ilqg, "almix", 0)
    (s,) = q.history("init")
    before = full_state(s)
    s.timing(True)
    for params in (None, {"lim": np.broadcast_to(np.asarray(q.params["lim"], dtype=np.float64), (B, np.size(q.params["lim"])))}):
        with pytest.raises(ilqg.IlqgError) as e:
            s.receding_plant(ROUNDS, steps, ITERATIONS, params=params)
        assert "ilqg_batch_receding_plant" in str(e.value) and "'%s'" % PER_STEP["almix"] in str(e.value) and "one value per time step" in str(e.value)
    with pytest.raises(ilqg.IlqgError) as e:
        s.receding_plant(ROUNDS, steps, ITERATIONS, params={PER_STEP["almix"]: np.zeros((B, q.N + 1))})
    assert PER_STEP["almix"] in str(e.value) and "per-time-step parameters stay shared" in str(e.value)
    assert s.kernel_times()["k_plant"][0] == 0
    assert_state_equal(full_state(s), before, "almix behind refused calls")
    q.close()
    # all outputs NULL is no no-op: the batch advances as it does with them, and n_names = 0 reads neither names nor values
    a.timing(True)
    raw(outputs=False)()
    assert a.kernel_times()["k_plant"][0] == ROUNDS * a.groups()
    want = b.receding_plant(ROUNDS, steps, ITERATIONS, True, X, rows, w)
    assert np.array_equal(xp, want["x_plant"]) and all(np.all(v == -7) for v in logs.values())
    assert_state_equal(full_state(a), full_state(b), "the batch behind a call without outputs")
    xp[:] = X
    raw(n_names=0, arr=None, values=None)()
    model = b.receding_plant(ROUNDS, steps, ITERATIONS, True, X, None, w)
    for k in ("x", "u", "cost", "plan_cost", "ok"):
        assert np.array_equal(logs[k], model[k]), k
    assert np.array_equal(xp, model["x_plant"])
    c.close()


# ---------------------------------------------------------------------------
# 7. a disturbance on every step of a round, against the reference's plant
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("feedback", [1, 0])
@pytest.mark.parametrize("name,strict", [(n, None) for n in ("carparking", "carparking_wave", "hxtest", "synth16x8", "synth10hx")] + [("synth16x8", True)])
def test_a_dense_disturbance_inside_a_round_equals_the_references_plant(ilqg, name, strict, feedback):
    """rounds = 1, steps = 4, a disturbance behind EVERY step: the read of the table at the steps before the last one,
    x_next + w, and the control of step k + 1 from the disturbed state.  x, u, the applied cost and x_plant against
    policy_cases.reference_plant under the plant's parameters."""
    steps = 4
    c = Case(ilqg, name, 0, count=2, strict=strict)
    a, b = c.history("init")
    table, rows = plant_rows(c)
    X, w = plant_starts(c), noise(c, steps, rounds=1)
    assert np.all(w != 0.0)
    out = a.receding_plant(1, steps, ITERATIONS, bool(feedback), X, rows, w)
    what = "%s strict=%s feedback=%d" % (name, strict, feedback)
    dev = hold_rounds(c, out, b, lambda s: params_of(c.params, table, s, 1), X, w, 1, steps, feedback, what)
    print(what + ": dense disturbance, worst deviation from the reference's plant " + ", ".join("%s %.3g" % kv for kv in dev.items()))
    c.close()


# ---------------------------------------------------------------------------
# 8. three rounds, teacher-forced on the device's own plant states
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["carparking", "synth16x8"])
def test_three_rounds_equal_the_references_plant_round_by_round(ilqg, name):
    """steps = 2, a disturbance behind every step, feedback: every round's x, u and applied cost, and the state the next
    round starts from, against the reference's plant from the state the DEVICE's plant had at the round's start about the
    policy a twin batch has there (hold_rounds); the plans' costs are the twin's bit for bit."""
    steps = 2
    c = Case(ilqg, name, 0, count=2)
    a, b = c.history("init")
    table, rows = plant_rows(c)
    X, w = plant_starts(c), noise(c, steps)
    out = a.receding_plant(ROUNDS, steps, ITERATIONS, True, X, rows, w)
    dev = hold_rounds(c, out, b, lambda s: params_of(c.params, table, s, 1), X, w, ROUNDS, steps, 1, name)
    assert_state_equal(full_state(a), full_state(b), "%s: the batch behind the loop against the teacher-forced twin" % name)
    print("%s: three rounds, worst deviation from the reference's plant " % name + ", ".join("%s %.3g" % kv for kv in dev.items()))
    c.close()


# ---------------------------------------------------------------------------
# 9. the largest step count the entry accepts
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("steps", [SHORT_N - 1, 1])
def test_the_largest_step_count_equals_the_references_plant(ilqg, steps):
    """CarParking with n_hor = 6, steps = n_hor - 1 = 5 (the plant applies every control of the plan but the last; the
    prefetch of step k + 1's nominal data reaches the plan's last step) and steps = 1 at the same horizon: two rounds, a
    disturbance behind every step, feedback, round by round against the reference's plant (hold_rounds)."""
    rounds = 2
    c = ShortCase(ilqg, count=2)
    assert c.N == SHORT_N and steps < c.N
    a, b = c.history("init")
    table, rows = plant_rows(c)
    X, w = plant_starts(c), noise(c, steps, rounds=rounds)
    out = a.receding_plant(rounds, steps, ITERATIONS, True, X, rows, w)
    what = "carparking n_hor=%d steps=%d" % (c.N, steps)
    dev = hold_rounds(c, out, b, lambda s: params_of(c.params, table, s, 1), X, w, rounds, steps, 1, what)
    assert_state_equal(full_state(a), full_state(b), what + ": the batch behind the loop against the teacher-forced twin")
    print(what + ": worst deviation from the reference's plant " + ", ".join("%s %.3g" % kv for kv in dev.items()))
    c.close()


def test_the_largest_step_count_equals_the_public_composition_bit_for_bit(ilqg):
    """test 2's composition in the FMA-free CarParking build at n_hor = 6, steps = 5, three rounds, the disturbance on each
    round's last step only (policy_rollout has none inside a roll-out): logs, x_plant and the batch afterwards bit for bit"""
    steps = SHORT_N - 1
    c = ShortCase(ilqg, count=2, strict=True)
    a, b = c.history("init")
    _, rows = plant_rows(c)
    X, w = plant_starts(c), noise(c, steps, last_only=True)
    out = a.receding_plant(ROUNDS, steps, ITERATIONS, True, X, rows, w)
    assert np.all(out["ok"] == 1)
    want = composition(b, rows, X, w, ROUNDS, steps)
    outputs_equal(out, want, "n_hor = %d, steps = %d: one call against the composition, FMA-free build" % (c.N, steps), sorted(want))
    assert_state_equal(full_state(a), full_state(b), "n_hor = %d, steps = %d: the batch behind the loop" % (c.N, steps))
    c.close()
