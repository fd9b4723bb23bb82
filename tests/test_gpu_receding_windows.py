"""BatchSolver.receding(windows=...) / receding_plant(windows=...) and MultiSolver.receding_plant(windows=...) on the GPU: the
resident closed loops for problems with per-time-step parameters, whose windows move with the horizon inside the loop
(ilqg_batch_receding_windows, ilqg_batch_receding_plant_windows, ilqg_multi_receding_plant_windows; k_shift_windows).

Cases are those of tests/window_loop_cases.py (B = 70, SLOTS 0, 63, 64, 69; a track per trajectory that goes on beyond the
horizon, rows = its first n_hor + 1 values, futures = the rest; rounds = steps = iterations = 3 unless stated), which
tests/test_receding_windows_recipe.py shows on the CPU to tell a moved window from an unmoved one and time index k from time
index 0 by 1e4 bars or more.  Tests 2 and 3 hold the loops against the oracle driver under the window the slot has in that
round (and, for the plant, at that step) with the tree's single-pass bar |d| <= 1e-10 max(1, |ref|); every other test is an
identity between calls of the product — the same kernels plus pure copies — and is bit for bit."""
import ctypes as C

import numpy as np
import pytest

from oracle.harness import Driver, lib_path
from policy_cases import shifted
from test_gpu_params_batch import launches, refused, states_equal
from test_gpu_policy_rollout import ilqg, worst  # noqa: F401 (fixture)
from test_gpu_receding_plant import full_state, plan_of
from params_batch_cases import oracle_stages
from window_loop_cases import BUILDS, ITERATIONS, ROUNDS, SLOTS, STEPS, B, WindowCase, close, dict_at, noise, plant_chain, plant_starts, track, window

pytestmark = pytest.mark.gpu

LOGS = ("x", "u", "cost")
PLANT_LOGS = ("x", "u", "cost", "plan_cost", "ok", "x_plant")


def cut(future, lo, hi):
    return None if future is None else np.ascontiguousarray(future[..., lo:hi])


def move(s, step, form, steps, tail):
    (s.shift_param_batch if form == "rows" else s.shift_param)(step, steps, tail)


def hand_loop(s, step, form, future, rounds, steps, iterations, first=0):
    """rounds x { iterate; head; shift_param_batch or shift_param with the round's tail; shift }: what receding(windows=...) is"""
    xs, us, cs = [], [], []
    for r in range(first, first + rounds):
        s.iterate(iterations)
        h = s.head(steps)
        xs.append(h["x"]), us.append(h["u"]), cs.append(h["cost"])
        move(s, step, form, steps, cut(future, r * steps, (r + 1) * steps))
        s.shift(steps)
    return dict(x=np.concatenate(xs, axis=1), u=np.concatenate(us, axis=1), cost=np.stack(cs, axis=1))


def hand_plant_loop(s, step, form, future, X, w, rounds, steps, iterations, feedback=True):
    """rounds x { iterate; policy_rollout from the plants' states, alpha = 0, whole roll-outs; x, u of the first `steps` steps;
    x_plant = x[steps] + w of the round's LAST step (policy_rollout has no disturbance inside a roll-out); the window moves;
    shift(steps, x0 = x_plant) }: what receding_plant(windows=...) is, up to the applied cost"""
    xp, xs, us, pc = X.copy(), [], [], []
    for r in range(rounds):
        s.iterate(iterations)
        pc.append(s.scalar("cost"))
        o = s.policy_rollout(xp[:, None], 0.0, feedback, trajectories=True)
        assert np.all(o["ok"] == 1)
        xs.append(o["x"][:, 0, 0:steps]), us.append(o["u"][:, 0, 0:steps])
        xp = o["x"][:, 0, steps] + (0.0 if w is None else w[:, r * steps + steps - 1])
        move(s, step, form, steps, cut(future, r * steps, (r + 1) * steps))
        s.shift(steps, x0=np.ascontiguousarray(xp))
    return dict(x=np.concatenate(xs, axis=1), u=np.concatenate(us, axis=1), plan_cost=np.stack(pc, axis=1), x_plant=xp)


def joined(parts, keys=LOGS):
    return {k: np.concatenate([p[k] for p in parts], axis=1) for k in keys}


def same(a, b, what, keys):
    for k in keys:
        assert np.array_equal(np.asarray(a[k]), np.asarray(b[k])), "%s: %s differs" % (what, k)


def futures_of(c, form, b=0):
    """(windows dict value, the future as the hand loop cuts it)"""
    if form == "rows":
        return c.future, c.future
    if form == "shared":
        return np.ascontiguousarray(c.future[b]), np.ascontiguousarray(c.future[b])
    return None, None


# ---------------------------------------------------------------------------
# 1. the loop is its composition, bit for bit
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["rows", "shared", "hold"])
@pytest.mark.parametrize("name,fd,strict", BUILDS)
def test_the_loop_is_its_composition(ilqg, name, fd, strict, form):
    """three batches with the same start: one call of 3 rounds and then one of 6; three calls of 3; and 9 rounds of
    { iterate; head; shift_param_batch or shift_param; shift } by hand.  rows: a window and a future per trajectory; shared:
    slot 63's window and future for all; hold: rows, the future None (named) or left out ({}).  Logs, the batch and the
    windows afterwards, and the batch two iterations later — for the shared window also behind a set_param of ANOTHER parameter,
    which re-sends every window from the host's copy."""
    R = ROUNDS
    c = WindowCase(ilqg, name, fd, strict, count=3, rounds=3 * R)
    a, b, h = c.start("shared" if form == "shared" else "rows", b=63)
    given, future = futures_of(c, form, b=63)
    hand_form = "shared" if form == "shared" else "rows"

    def call(s, r0, rounds, named=True):
        w = {c.step: cut(given, r0 * STEPS, (r0 + rounds) * STEPS)} if named else {}
        return s.receding(rounds, STEPS, ITERATIONS, windows=w)

    one = joined([call(a, 0, R), call(a, R, 2 * R, named=form != "hold")])
    three = joined([call(b, 0, R), call(b, R, R, named=form != "hold"), call(b, 2 * R, R)])
    hand = hand_loop(h, c.step, hand_form, future, 3 * R, STEPS, ITERATIONS)
    what = "%s fd%d%s %s" % (name, fd, " FMA-free" if strict else "", form)
    same(one, hand, what + ": the loop against the hand loop", LOGS)
    same(three, one, what + ": three calls of three rounds against calls of three and six", LOGS)
    assert one["x"].shape == (B, 9 * STEPS, a.problem.nx) and one["cost"].shape == (B, 9)
    moved = 3 * R * STEPS
    if form == "rows":
        want = window(c.T, c.N, moved)
    elif form == "shared":
        want = np.tile(window(c.T[63], c.N, moved), (B, 1))
    else:
        want = np.concatenate([c.rows[:, moved:], np.repeat(c.rows[:, -1:], moved, axis=1)], axis=1)
    for s, who in ((a, "the loop"), (b, "three calls"), (h, "the hand loop")):
        assert np.array_equal(s.param_steps_batch(c.step), want), "%s: the windows behind %s" % (what, who)
    states_equal(full_state(a), full_state(h), what + ": the batch behind the loop")
    states_equal(full_state(b), full_state(h), what + ": the batch behind three calls")
    other = next(k for k, size in a.problem.params if size > 0)
    for s in (a, b, h):
        if form == "shared":
            s.set_param(other, c.params[other])  # (every window goes up again, from the host's copy)
            s.shift(0)
        s.iterate(2)
    states_equal(full_state(a), full_state(h), what + ": two iterations behind the loop")
    states_equal(full_state(b), full_state(h), what + ": two iterations behind three calls")
    c.close()


# ---------------------------------------------------------------------------
# 2. the moved window against the reference
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("fd", [0, 1])
def test_every_round_plans_under_the_moved_window_of_its_slot(ilqg, fd):
    """brachi_hli, rows, iterations = 0: the plan of round r is the initial roll-out from x_applied[b, r * steps] with the
    controls shifted by r * steps under the window that begins r * steps values into slot b's track.  Its cost and its first
    `steps` states against the oracle driver under that dict; behind the loop x() and the cost against oracle_stages under the
    window rounds * steps on.  (The recipe test: under the UNMOVED window the cost is off by 4e9 bars.)"""
    name = "brachi_hli"
    c = WindowCase(ilqg, name, fd)
    (s,) = c.start("rows")
    out = s.receding(ROUNDS, STEPS, 0, windows={c.step: c.future})
    lib = lib_path("oracle", name, fd)
    dev = dict(cost=0.0, x=0.0)
    for b in SLOTS:
        for r in range(ROUNDS):
            d = Driver(lib, c.N, dict_at(name, c.params, c.T, c.N, b, r * STEPS), c.opts)
            assert d.init(out["x"][b, r * STEPS], shifted(c.u0[b], r * STEPS)) == 1
            cost, (x, _) = d.scalars()["cost"], d.traj(0)
            d.close()
            got = dict(cost=out["cost"][b, r], x=out["x"][b, r * STEPS:(r + 1) * STEPS])
            want = dict(cost=cost, x=x[:STEPS])
            for k in got:
                dev[k] = max(dev[k], worst(got[k], want[k]))
                assert close(got[k], want[k]), "fd%d slot %d round %d: %s off by %.3g" % (fd, b, r, k, worst(got[k], want[k]))
    x, cost, status = s.x(), s.scalar("cost"), s.ints("status")
    for b in SLOTS:
        ref = oracle_stages(lib, c.N, dict_at(name, c.params, c.T, c.N, b, ROUNDS * STEPS), c.opts, x[b, 0], shifted(c.u0[b], ROUNDS * STEPS))
        assert ref["init"] == 1 and status[b] == 0
        for k, got, want in (("x behind the loop", x[b], ref["x"]), ("cost behind the loop", cost[b], ref["cost"])):
            dev[k] = max(dev.get(k, 0.0), worst(got, want))
            assert close(got, want), "fd%d slot %d: %s off by %.3g" % (fd, b, k, worst(got, want))
    assert np.array_equal(s.param_steps_batch(c.step), window(c.T, c.N, ROUNDS * STEPS))
    print("brachi_hli fd%d: worst deviation from the oracle under the moved windows: " % fd + ", ".join("%s %.3g" % kv for kv in dev.items()))
    c.close()


# ---------------------------------------------------------------------------
# 3. the plant's steps against the reference
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("rounds", [1, ROUNDS])
@pytest.mark.parametrize("strict", [False, True])
def test_the_plants_steps_read_the_slots_window_at_their_own_time_index(ilqg, strict, rounds):
    """almix FULL_DDP 1, feedback, a disturbance behind every step; the rounds teacher-forced on the device's own plant states
    and on the plans of a twin batch that runs the hand loop.  Step k of round r against a one-step roll-out of the oracle
    under slot b's window r * steps + k on, the policy and the running multipliers shifted by k (window_loop_cases.plant_chain).
    In almix only the cost depends on `vref`: the applied cost is the output that tells (the recipe test: at time index 0 it
    is off by 1e6 bars or more in every round)."""
    name, fd = "almix", 1
    c = WindowCase(ilqg, name, fd, strict, count=2)
    a, twin = c.start("rows")
    X, w = plant_starts(c.x0), noise(c.x0.shape[1], STEPS)
    out = a.receding_plant(rounds, STEPS, ITERATIONS, True, X, None, w[:, :rounds * STEPS], windows={c.step: c.future[:, :rounds * STEPS]})
    assert np.all(out["ok"] == 1)
    lib = lib_path("oracle", name, fd)
    dev = dict(x=0.0, u=0.0, cost=0.0, x_plant=0.0)
    Xr = X
    for r in range(rounds):
        twin.iterate(ITERATIONS)
        plan = plan_of(twin)
        assert np.array_equal(out["plan_cost"][:, r], twin.scalar("cost")), "round %d: the plans' costs are not the twin's" % r
        lo, hi = r * STEPS, (r + 1) * STEPS
        nxt = out["x"][:, hi] if r + 1 < rounds else out["x_plant"]
        for b in SLOTS:
            policy, kw = plan(b)
            x, u, _, cost, x_end = plant_chain(lib, name, c.N, c.params, c.T, b, lo, c.opts, Xr[b], policy, 1, STEPS, w=w[b, lo:hi], **kw)
            assert all(np.all(np.isfinite(v)) for v in (x, u, cost, x_end)), "round %d slot %d: the reference is not finite" % (r, b)
            got = dict(x=out["x"][b, lo:hi], u=out["u"][b, lo:hi], cost=out["cost"][b, r], x_plant=nxt[b])
            want = dict(x=x, u=u, cost=cost, x_plant=x_end)
            for k in got:
                dev[k] = max(dev[k], worst(got[k], want[k]))
            for k in got:
                assert close(got[k], want[k]), "strict=%s round %d slot %d: %s off by %.3g" % (strict, r, b, k, worst(got[k], want[k]))
        twin.shift_param_batch(c.step, STEPS, np.ascontiguousarray(c.future[:, lo:hi]))
        twin.shift(STEPS, x0=np.ascontiguousarray(nxt))
        Xr = nxt
    states_equal(full_state(a), full_state(twin), "the batch behind the loop against the teacher-forced twin")
    assert np.array_equal(a.param_steps_batch(c.step), twin.param_steps_batch(c.step))
    print("almix fd1%s, %d round(s): worst deviation from the reference's plant under the moving windows " % (" FMA-free" if strict else "", rounds) +
          ", ".join("%s %.3g" % kv for kv in dev.items()))
    c.close()


# ---------------------------------------------------------------------------
# 4. the plant loop is its composition
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("steps,disturbed", [(1, True), (3, False)])
def test_the_plant_loop_is_its_composition(ilqg, steps, disturbed):
    """FMA-free almix, rows: one call against { iterate; policy_rollout(x_plant, 0.0, feedback, trajectories); shift_param_batch;
    shift(x0 = x_plant) }: x, u, the plans' costs, the plants' states and the batch afterwards bit for bit.  steps = 1 with a
    disturbance (policy_rollout has none inside a roll-out), steps = 3 without."""
    c = WindowCase(ilqg, "almix", 1, True, count=2, steps=steps)
    a, b = c.start("rows")
    X = plant_starts(c.x0)
    w = noise(c.x0.shape[1], steps) if disturbed else None
    out = a.receding_plant(ROUNDS, steps, ITERATIONS, True, X, None, w, windows={c.step: c.future})
    assert np.all(out["ok"] == 1)
    want = hand_plant_loop(b, c.step, "rows", c.future, X, w, ROUNDS, steps, ITERATIONS)
    same(out, want, "steps = %d: one call against the composition" % steps, sorted(want))
    states_equal(full_state(a), full_state(b), "steps = %d: the batch behind the loop" % steps)
    assert np.array_equal(a.param_steps_batch(c.step), window(c.T, c.N, ROUNDS * steps))
    assert np.array_equal(b.param_steps_batch(c.step), window(c.T, c.N, ROUNDS * steps))
    c.close()


# ---------------------------------------------------------------------------
# 5. block boundaries
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["rows", "shared"])
@pytest.mark.parametrize("steps", [1, 255, 256, 257])
def test_windows_of_three_blocks_move_by_a_block_more_or_less(ilqg, steps, form):
    """brachi_hli at n_hor = 600 (a window of 601 values spans three blocks of k_shift_windows), iterations = 0, two rounds: the
    windows afterwards are the track 2 * steps on bit for bit, and the loop is the hand loop"""
    rounds = 2
    c = WindowCase(ilqg, "brachi_hli", 0, count=2, n=600, rounds=rounds, steps=steps)
    assert c.N == 600 and c.T.shape == (B, 601 + rounds * steps)
    a, h = c.start(form, b=64)
    given, future = futures_of(c, form, b=64)
    out = a.receding(rounds, steps, 0, windows={c.step: given})
    hand = hand_loop(h, c.step, form, future, rounds, steps, 0)
    want = window(c.T, c.N, rounds * steps) if form == "rows" else np.tile(window(c.T[64], c.N, rounds * steps), (B, 1))
    assert np.array_equal(a.param_steps_batch(c.step), want), "steps = %d %s: the windows behind the loop" % (steps, form)
    assert np.array_equal(h.param_steps_batch(c.step), want)
    same(out, hand, "steps = %d %s: the loop against the hand loop" % (steps, form), LOGS)
    states_equal(full_state(a), full_state(h), "steps = %d %s: the batch behind the loop" % (steps, form))
    c.close()


# ---------------------------------------------------------------------------
# 6. invariance to layout
# ---------------------------------------------------------------------------
def plant_run(s, c, X, w, flip=False):
    def f(v):
        return np.ascontiguousarray(v[::-1]) if flip else v
    s.set_param_steps_batch(c.step, f(c.rows))
    s.init(f(c.x0), f(c.u0))
    return s.receding_plant(c.rounds, c.steps, ITERATIONS, True, f(X), None, f(w), windows={c.step: f(c.future)})


def test_groups_shards_and_the_reversed_batch_give_the_same_bits(ilqg):
    """B = 200 is four stream groups of 64 (the last one ragged): groups 1 / 2 / 4 and two loop-back shards of a MultiSolver,
    every group and shard with its rows of the futures; then the reversed batch at B = 70.  almix FULL_DDP 1, the plant loop
    with feedback and a disturbance, and the model loop beside it for the groups."""
    n = 200
    cases = [WindowCase(ilqg, "almix", 1, groups=g, batch=n, count=2) for g in (1, 2, 4)]
    c = cases[0]
    X, w = plant_starts(c.x0), noise(c.x0.shape[1], STEPS, batch=n)
    outs = []
    for q in cases:
        s, t = q.solvers
        plant = plant_run(s, q, X, w)
        t.set_param_steps_batch(q.step, q.rows)
        t.init(q.x0, q.u0)
        model = t.receding(ROUNDS, STEPS, ITERATIONS, windows={q.step: q.future})
        outs.append((plant, full_state(s), s.param_steps_batch(q.step), model, full_state(t), t.param_steps_batch(q.step)))
    assert np.all(outs[0][0]["ok"] == 1)
    for g, o in zip((2, 4), outs[1:]):
        same(o[0], outs[0][0], "%d stream groups against one: the plant loop" % g, PLANT_LOGS)
        same(o[3], outs[0][3], "%d stream groups against one: the model loop" % g, LOGS)
        states_equal(o[1], outs[0][1], "%d stream groups against one: the batch behind the plant loop" % g)
        states_equal(o[4], outs[0][4], "%d stream groups against one: the batch behind the model loop" % g)
        assert np.array_equal(o[2], outs[0][2]) and np.array_equal(o[5], outs[0][5])
    assert np.array_equal(outs[0][2], window(c.T, c.N, ROUNDS * STEPS))
    m = ilqg.MultiSolver("almix", 1, batch=n, n_hor=c.N, devices=[0, 0], params=c.params, opts=dict(c.opts, max_iter=40))
    same(plant_run(m, c, X, w), outs[0][0], "two shards against the single batch", PLANT_LOGS)
    base = outs[0][1]
    assert np.array_equal(m.x(), base["x"]) and np.array_equal(m.u(), base["u"])
    assert np.array_equal(m.ints("iterations"), base["iterations"]) and np.array_equal(m.ints("status"), base["status"])
    m.close()
    for q in cases:
        q.close()
    c = WindowCase(ilqg, "almix", 1, count=2)
    X, w = plant_starts(c.x0), noise(c.x0.shape[1], STEPS)
    a, b = c.solvers
    fwd, rev = plant_run(a, c, X, w), plant_run(b, c, X, w, flip=True)
    same({k: v[::-1] for k, v in rev.items()}, fwd, "the reversed batch", PLANT_LOGS)
    states_equal({k: v[::-1] for k, v in full_state(b).items()}, full_state(a), "the reversed batch: the batch behind the loop")
    assert np.array_equal(b.param_steps_batch(c.step)[::-1], a.param_steps_batch(c.step))
    c.close()


# ---------------------------------------------------------------------------
# 7. no host round trip
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["rows", "shared"])
def test_one_launch_per_round_and_group_moves_every_window(ilqg, form):
    """the launches by kernel over one call of each of the four forms of the resident loop, g the solver's stream groups: the
    round's record is k_log_steps (receding) or k_plant (receding_plant), never both, rounds x g of it; k_shift rounds x g;
    k_shift_windows rounds x g in the windowed forms and none in the others; and not one k_shift_param / k_shift_param_rows —
    the loop does not go through the entries that stage a tail from the host.
    Shapes: receding / receding_plant on CarParking FULL_DDP 0, n_hor = 6; the windowed forms on almix FULL_DDP 1, n_hor = 8,
    `vref` with rows per trajectory or shared (`form`); rounds = 3, steps = 1 and 5, one iteration a round; groups = 1 and 2
    asked for at B = 9 — where a stream group is whole tiles of 64 trajectories, so both are ONE group and g = 1 (the 5 + 4
    split of nine trajectories is MultiSolver's, over shards, and a shard is a batch of its own) — and at B = 73 = 64 + 9, the
    smallest batch at which two groups exist."""
    from oracle.harness import CAR_PARAMS, almix_case
    from conftest import load_package
    rounds, n_car, n_mix = 3, 6, 8
    names = ("k_log_steps", "k_plant", "k_shift", "k_shift_windows", "k_shift_param", "k_shift_param_rows")

    def counted(s, call):
        before = launches(s)
        call()
        after = launches(s)
        return {k: after[k] - before[k] for k in names}

    for batch, groups in ((9, 1), (9, 2), (73, 1), (73, 2)):
        x0, u0 = load_package().synth.car_batch(batch, n_car, first=40)
        params, opts, y0, v0 = almix_case(batch=batch)
        v0 = np.ascontiguousarray(v0[:, :n_mix])
        vref = 0.8 + 0.4 * np.sin(0.2 * np.arange(n_mix + 1 + rounds * 5))
        tracks = np.ascontiguousarray(vref[None, :] * (1.0 + 0.05 * np.random.default_rng(59).standard_normal((batch, vref.size))))
        car = ilqg.BatchSolver("carparking", 0, batch=batch, n_hor=n_car, params=CAR_PARAMS, opts=dict(max_iter=40), groups=groups)
        mix = ilqg.BatchSolver("almix", 1, batch=batch, n_hor=n_mix, params=dict(params, vref=vref[:n_mix + 1]), opts=dict(opts, max_iter=40), groups=groups)
        assert car.groups() == mix.groups() == (groups if batch > 64 else 1)
        g = car.groups()
        car.timing(True), mix.timing(True)
        for steps in (1, 5):
            more = slice(n_mix + 1, n_mix + 1 + rounds * steps)
            given = np.ascontiguousarray(tracks[:, more] if form == "rows" else vref[more])

            def start_mix():
                if form == "rows":
                    mix.set_param_steps_batch("vref", tracks[:, :n_mix + 1])
                else:
                    mix.set_param("vref", vref[:n_mix + 1])
                mix.init(y0, v0)

            got = {}
            car.init(x0, u0)
            got["receding"] = counted(car, lambda: car.receding(rounds, steps, 1))
            car.init(x0, u0)
            got["receding_plant"] = counted(car, lambda: car.receding_plant(rounds, steps, 1, True))
            start_mix()
            got["receding, windows"] = counted(mix, lambda: mix.receding(rounds, steps, 1, windows=dict(vref=given)))
            start_mix()
            got["receding_plant, windows"] = counted(mix, lambda: mix.receding_plant(rounds, steps, 1, True, windows=dict(vref=given)))
            for what, n in got.items():
                plant, windowed = "plant" in what, "windows" in what
                want = dict(k_log_steps=0 if plant else rounds * g, k_plant=rounds * g if plant else 0, k_shift=rounds * g,
                            k_shift_windows=rounds * g if windowed else 0, k_shift_param=0, k_shift_param_rows=0)
                assert n == want, "%s, B = %d, %d group(s), steps = %d: launches %r, expected %r" % (what, batch, g, steps, n, want)
        car.close(), mix.close()


# ---------------------------------------------------------------------------
# 8. the empty case
# ---------------------------------------------------------------------------
def strings(*words):
    return (C.c_char_p * max(len(words), 1))(*[v.encode() for v in words])


def pointers(*arrays):
    return (C.c_void_p * max(len(arrays), 1))(*[None if a is None else a.ctypes.data for a in arrays])


def ptr(a):
    return None if a is None else C.c_void_p(a.ctypes.data)


def test_a_problem_without_windows_runs_the_old_loops_bit_for_bit(ilqg):
    from test_gpu_policy_rollout import Case
    from plant_cases import noise as car_noise, plant_rows, plant_starts as car_starts
    c = Case(ilqg, "carparking", 0, count=4)
    a, b, p, q = c.history("init")
    same(a.receding(ROUNDS, STEPS, 2, windows={}), b.receding(ROUNDS, STEPS, 2), "receding(windows={}) against receding()", LOGS)
    states_equal(full_state(a), full_state(b), "the batch behind receding(windows={})")
    _, rows = plant_rows(c)
    X, w = car_starts(c), car_noise(c, STEPS)
    same(p.receding_plant(ROUNDS, STEPS, 2, True, X, rows, w, windows={}), q.receding_plant(ROUNDS, STEPS, 2, True, X, rows, w),
         "receding_plant(windows={}) against receding_plant()", PLANT_LOGS)
    states_equal(full_state(p), full_state(q), "the batch behind receding_plant(windows={})")
    # a window on a problem that has none
    f = np.zeros(ROUNDS * STEPS)
    x = np.zeros((B, ROUNDS * STEPS, c.nx))
    refused(ilqg, a, lambda: a.receding(ROUNDS, STEPS, 2, windows=dict(cx=None)), ("receding", "cx", "fixed size"))
    refused(ilqg, a, lambda: a.receding(ROUNDS, STEPS, 2, windows=dict(vref=f)), ("receding", "Parameter name 'vref' is not member of parameters struct."))
    refused(ilqg, a, lambda: a._ck(a.lib.ilqg_batch_receding_windows(a.h, ROUNDS, STEPS, 2, 1, strings("cx"), pointers(f), ptr(x), None, None)),
            ("ilqg_batch_receding_windows", "n_windows = 1", "no parameter with one value per time step"))
    refused(ilqg, p, lambda: p._ck(p.lib.ilqg_batch_receding_plant_windows(p.h, ROUNDS, STEPS, 2, 1, None, 0, None, None, None, 1, strings("cx"), pointers(f),
                                                                             ptr(x), None, None, None, None)),
            ("ilqg_batch_receding_plant_windows", "n_windows = 1", "no parameter with one value per time step"))
    assert np.all(x == 0.0)
    c.close()


# ---------------------------------------------------------------------------
# 9. failure stays in its slot
# ---------------------------------------------------------------------------
def test_a_nan_in_one_future_fails_its_own_slot_only(ilqg):
    """a NaN — data, not a fault — in slot 64's future at the first column of round 1.  The model loop at n_hor = 80: the value
    enters the window's end behind round 1 and the initial roll-out of the shift meets it: status != 0 for that slot alone.
    The plant loop at n_hor = 8, five rounds: the value reaches time index 0 of the window behind round 3, where the first step
    of round 4's plant reads it (if the failed plan has not stopped the plant before): ok = 0 for that slot alone.  Every other slot keeps the bits of the clean run."""
    keep = np.arange(B) != 64
    c = WindowCase(ilqg, "almix", 1, count=2)
    good, bad = c.start("rows")
    broken = c.future.copy()
    broken[64, STEPS] = np.nan
    clean = good.receding(ROUNDS, STEPS, ITERATIONS, windows={c.step: c.future})
    got = bad.receding(ROUNDS, STEPS, ITERATIONS, windows={c.step: broken})
    st = bad.ints("status")
    print("status of the slot with the NaN behind the model loop: %d" % st[64])
    assert st[64] != 0 and np.all(st[keep] == 0) and np.all(good.ints("status") == 0)
    for k in LOGS:
        assert np.array_equal(got[k][keep], clean[k][keep]), k
    states_equal(full_state(bad), full_state(good), "every other slot beside the NaN future", keep, keep)
    c.close()
    # the plant loop on a short horizon
    n, rounds = 8, 5
    from oracle.harness import almix_case
    params, opts, x0, u0 = almix_case(batch=B)
    params = dict(params, vref=np.asarray(params["vref"])[:n + 1])
    u0 = np.ascontiguousarray(u0[:, :n])
    T = track("almix", params, n, rounds, STEPS)
    rows, future = window(T, n, 0), np.ascontiguousarray(T[:, n + 1:])
    broken = future.copy()
    broken[64, STEPS] = np.nan
    X = plant_starts(x0)
    outs = []
    for f in (future, broken):
        s = ilqg.BatchSolver("almix", 1, batch=B, n_hor=n, params=params, opts=dict(opts, max_iter=40))
        s.set_param_steps_batch("vref", rows)
        s.init(x0, u0)
        outs.append((s.receding_plant(rounds, STEPS, 1, True, X, windows=dict(vref=f)), full_state(s)))
        s.close()
    (clean, state_clean), (got, state_got) = outs
    assert got["ok"][64] == 0 and np.all(got["ok"][keep] == 1) and np.all(clean["ok"] == 1)
    for k in PLANT_LOGS:
        assert np.array_equal(got[k][keep], clean[k][keep]), k
    states_equal(state_got, state_clean, "every other slot beside the NaN future, plant loop", keep, keep)


# ---------------------------------------------------------------------------
# 10. refusals: the error text, an untouched batch and untouched windows, no launch
# ---------------------------------------------------------------------------
def test_refusals_leave_the_batch_and_the_windows_untouched(ilqg):
    c = WindowCase(ilqg, "almix", 1, count=2)
    s, t = c.start("rows")
    for q in (s, t):
        q.iterate(2)
    lib, h = s.lib, s.h
    n = ROUNDS * STEPS
    logs = dict(x=np.full((B, n, 3), -7.0), u=np.full((B, n, 2), -7.0), cost=np.full((B, ROUNDS), -7.0), plan_cost=np.full((B, ROUNDS), -7.0),
                ok=np.full(B, -7, dtype=np.int32))
    f = c.future
    lim = np.ascontiguousarray(np.broadcast_to(np.asarray(c.params["lim"], dtype=np.float64), (B, 2)))

    def model(rounds=ROUNDS, steps=STEPS, iterations=ITERATIONS, n_windows=1, names=strings("vref"), future=pointers(f)):
        return lambda: s._ck(lib.ilqg_batch_receding_windows(h, rounds, steps, iterations, n_windows, names, future,
                                                             *[ptr(logs[k]) for k in ("x", "u", "cost")]))

    def plant(rounds=ROUNDS, steps=STEPS, iterations=ITERATIONS, n_names=0, arr=None, values=None, n_windows=1, names=strings("vref"), future=pointers(f)):
        return lambda: s._ck(lib.ilqg_batch_receding_plant_windows(h, rounds, steps, iterations, 1, None, n_names, arr, ptr(values), None, n_windows, names,
                                                                   future, *[ptr(logs[k]) for k in ("x", "u", "cost", "plan_cost", "ok")]))

    for make, entry in ((model, "ilqg_batch_receding_windows"), (plant, "ilqg_batch_receding_plant_windows")):
        # what the old entries refuse
        for r in (0, -1):
            refused(ilqg, s, make(rounds=r), (entry, "rounds"))
        refused(ilqg, s, make(iterations=-1), (entry, "iterations"))
        for k in (0, -1, c.N, c.N + 5):
            refused(ilqg, s, make(steps=k), (entry, "steps", "n_hor"))
        # the windows
        refused(ilqg, s, make(n_windows=-1), (entry, "n_windows = -1"))
        refused(ilqg, s, make(names=None), (entry, "window_names is NULL"))
        refused(ilqg, s, make(future=None), (entry, "future is NULL"))
        refused(ilqg, s, make(names=strings("nope")), (entry, "window_names[0]", "Parameter name 'nope' is not member of parameters struct."))
        refused(ilqg, s, make(names=strings("tgt")), (entry, "window_names[0]", "tgt", "fixed size of 3"))
        refused(ilqg, s, make(n_windows=2, names=strings("vref", "vref"), future=pointers(f, f)), (entry, "window_names[1]", "vref", "twice"))
    # the plant's own names: what ilqg_batch_receding_plant refuses, a per-time-step name among them
    refused(ilqg, s, plant(n_names=-1), ("ilqg_batch_receding_plant_windows", "n_names"))
    refused(ilqg, s, plant(n_names=1, arr=None, values=lim), ("ilqg_batch_receding_plant_windows", "names"))
    refused(ilqg, s, plant(n_names=1, arr=strings("lim"), values=None), ("ilqg_batch_receding_plant_windows", "values"))
    refused(ilqg, s, plant(n_names=1, arr=strings("nope"), values=lim), ("names[0]", "Parameter name 'nope' is not member of parameters struct."))
    refused(ilqg, s, plant(n_names=2, arr=strings("lim", "lim"), values=lim), ("names[1]", "lim", "twice"))
    refused(ilqg, s, plant(n_names=1, arr=strings("vref"), values=lim), ("names[0]", "vref", "one value per time step"))
    # the old entries keep their refusal
    refused(ilqg, s, lambda: s.receding(ROUNDS, STEPS, ITERATIONS), ("ilqg_batch_receding", "vref", "ilqg_batch_shift"))
    refused(ilqg, s, lambda: s.receding_plant(ROUNDS, STEPS, ITERATIONS), ("ilqg_batch_receding_plant", "vref", "ilqg_batch_shift"))
    # the binding refuses before the library: a future of the wrong form
    refused(ilqg, s, lambda: s.receding(ROUNDS, STEPS, ITERATIONS, windows=dict(vref=f[0])), ("receding", "windows['vref']", "shape"))
    assert all(np.all(v == -7) for v in logs.values()), "a refused call wrote an output"
    assert np.array_equal(s.param_steps_batch("vref"), c.rows), "a refused call moved a window"
    for q in (s, t):
        q.iterate(2)
    states_equal(full_state(s), full_state(t), "after the refusals")
    c.close()


# ---------------------------------------------------------------------------
# 11. the wave mapping
# ---------------------------------------------------------------------------
def test_the_wave_mapping_moves_its_shared_window(ilqg):
    """wave-mapped brachi_hli, batch 8: no rows there, the window is shared and so is its future.  The model loop against the
    hand loop with shift_param, and one call of the plant loop against a call per round, bit for bit; the constant entries of
    the derivative records follow the moved window (two iterations later the batches still agree)."""
    n = 8
    c = WindowCase(ilqg, "brachi_hli", 0, "wave", count=4, batch=n)
    a, h, p, q = c.start("shared", b=5)
    future = np.ascontiguousarray(c.future[5])
    out = a.receding(ROUNDS, STEPS, ITERATIONS, windows={c.step: future})
    hand = hand_loop(h, c.step, "shared", future, ROUNDS, STEPS, ITERATIONS)
    same(out, hand, "wave mapping: the loop against the hand loop", LOGS)
    one = p.receding_plant(ROUNDS, STEPS, ITERATIONS, False, windows={c.step: future})
    parts = [q.receding_plant(1, STEPS, ITERATIONS, False, windows={c.step: future[r * STEPS:(r + 1) * STEPS]}) for r in range(ROUNDS)]
    same(one, joined(parts, ("x", "u", "cost", "plan_cost")), "wave mapping: three rounds against three calls of one", ("x", "u", "cost", "plan_cost"))
    other = next(k for k, size in a.problem.params if size > 0)
    for s in (a, h, p, q):
        s.set_param(other, c.params[other])  # (every window goes up again, from the host's copy)
        s.shift(0)
        s.iterate(2)
    states_equal(full_state(a), full_state(h), "wave mapping: the batch behind the loop")
    states_equal(full_state(p), full_state(q), "wave mapping: the batch behind the plant loop")
    c.close()
