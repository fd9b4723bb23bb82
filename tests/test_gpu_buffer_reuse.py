"""Device buffers of a context that grow, or are made anew, while the context is alive: the second-stage candidates, the kept
roll-out planes, the per-trajectory table, the window futures with the log, and the plants.

Every case runs ONE scenario twice on the same library: (a) in a fresh solver, where the scenario itself makes the buffers grow,
and (b) in a solver that made every larger request of the scenario beforehand and was then put back to the scenario's start
(the options and parameters it begins with, init from the same x0, u0), so that nothing grows while it runs.  Both are the
same kernels on the same inputs: every output of every phase is compared with np.array_equal, in product builds.  From the
launch counts of kernel_times() each case also asserts that the path it is about is the one that ran.

Shapes: B = 70 (one full and one partly filled wavefront), N = 20, the standard eight step sizes, two iterations per phase;
CarParking FULL_DDP 0 for cases 1 to 3, almix FULL_DDP 1 (a parameter with a value per time step) for cases 4 and 5;
synth16x8 FULL_DDP 1 (wave mapping), B = 3, N = 6 for case 6."""
import numpy as np
import pytest

from oracle.harness import CAR_PARAMS, SYN_PARAMS_TIGHT, almix_case, syn_inputs
from policy_param_cases import NAMED, draws, limits_ordered
from test_gpu_params_batch import launches
from test_gpu_policy_rollout import ilqg  # noqa: F401 (fixture)

pytestmark = pytest.mark.gpu

B, N, ITERATIONS = 70, 20, 2
VREF_MORE = 12  # values of almix's `vref` beyond the window: the two loops of case 4 move it 2 x 1 + 5 x 2 on


def car(ilqg, **opts):
    from conftest import load_package
    x0, u0 = load_package().synth.car_batch(B, N, first=40)
    x0[B // 2:] *= 4.0  # (as tests/test_gpu_receding.py: the far starts are the ones that reach the second stage)
    u0[B // 2:] *= 10.0

    def make():
        return ilqg.BatchSolver("carparking", 0, batch=B, n_hor=N, params=CAR_PARAMS, opts=dict(max_iter=40, **opts))

    return make, x0, u0


def almix(ilqg):
    """(make, x0, u0, vref [N + 1 + VREF_MORE] shared, tracks [B, N + 1 + VREF_MORE] per trajectory, params)"""
    params, opts, x0, u0 = almix_case(batch=B)
    vref = 0.8 + 0.4 * np.sin(0.2 * np.arange(N + 1 + VREF_MORE))
    assert np.array_equal(vref[:N + 1], np.asarray(params["vref"])[:N + 1])
    params = dict(params, vref=vref[:N + 1])
    tracks = np.ascontiguousarray(vref[None, :] * (1.0 + 0.05 * np.random.default_rng(61).standard_normal((B, vref.size))))

    def make():
        return ilqg.BatchSolver("almix", 1, batch=B, n_hor=N, params=params, opts=dict(opts, max_iter=40))

    return make, x0, np.ascontiguousarray(u0[:, :N]), vref, tracks, params


def scalars(s):
    """what can be read without moving a trajectory (x() and u() bring every trajectory home from its plane)"""
    return dict(cost=s.scalar("cost"), alpha_idx=s.ints("alpha_idx"), accepted=s.ints("accepted"), status=s.ints("status"))


def snap(s):
    return dict(scalars(s), x=s.x(), u=s.u())


def same(a, b, what):
    assert len(a) == len(b)
    for i, (p, q) in enumerate(zip(a, b)):
        assert sorted(p) == sorted(q)
        for k in sorted(p):
            if p[k] is None or q[k] is None:
                assert p[k] is None and q[k] is None, "%s, output %d: %s is given in one run only" % (what, i, k)
                continue
            assert np.array_equal(np.asarray(p[k]), np.asarray(q[k])), "%s, output %d: %s differs" % (what, i, k)


def fresh_and_grown(make, start, grow, scenario, what):
    """the scenario in a fresh solver and in one that made the larger requests first; returns (outputs, launches) of the fresh one"""
    a, b = make(), make()
    try:
        start(a)
        grow(b)
        start(b)
        for s in (a, b):
            s.timing(True)
        out_a, out_b = scenario(a), scenario(b)
        n_a, n_b = launches(a), launches(b)
        same(out_a, out_b, what)
        assert n_a == n_b, "%s: the two runs launched different kernels" % what
        return out_a, n_a
    finally:
        a.close()
        b.close()


def split_phases(s, splits, last_with_trajectories=True):
    out = []
    for i, split in enumerate(splits):
        s.set_option("ls_split", split)
        s.iterate(ITERATIONS)
        out.append(snap(s) if last_with_trajectories and i == len(splits) - 1 else scalars(s))
    return out


# ---------------------------------------------------------------------------
# 1. the second-stage candidates of ls_keep = 1
# ---------------------------------------------------------------------------
def test_second_stage_candidates_grow_threefold(ilqg):
    """ls_keep = 1: ls_split = 6 (two step sizes in the second stage), then 2 (six): the candidates of ROLL_SECOND grow threefold
    between two iterations.  The path: one second-stage roll-out launch and one k_adopt per iteration, no k_search."""
    make, x0, u0 = car(ilqg, ls_keep=1)

    def start(s):
        s.set_option("ls_split", 6)
        s.init(x0, u0)

    def grow(s):
        s.set_option("ls_split", 2)
        s.init(x0, u0)
        s.iterate(1)

    out, n = fresh_and_grown(make, start, grow, lambda s: split_phases(s, (6, 2)), "candidates of the second stage")
    assert n["k_rollout[stage 2 | winner]"] == 2 * ITERATIONS and n["k_rollout[winner]"] == 2 * ITERATIONS
    assert n["k_search[stage 1]"] == 0 and n["k_search[stage 2]"] == 0
    assert np.all(np.isfinite(out[-1]["cost"]))


# ---------------------------------------------------------------------------
# 2. the kept roll-out planes of ls_keep = 2
# ---------------------------------------------------------------------------
def test_kept_planes_grow_and_trajectories_are_rehomed(ilqg):
    """ls_keep = 2: ls_split = 2, then 4 — the planes grow, plane_n changes and the trajectories that live in a plane go home first
    (nothing is read between the phases that would bring them home) — then 2 again.  With eight step sizes the first phase
    already has the six second-stage step sizes of the third, so a fourth phase, ls_split = 1 (seven), is what makes the
    candidates of k_search<1> grow behind a smaller buffer."""
    make, x0, u0 = car(ilqg, ls_keep=2)

    def start(s):
        s.set_option("ls_split", 2)
        s.init(x0, u0)

    def grow(s):
        s.init(x0, u0)
        for split in (4, 1):
            s.set_option("ls_split", split)
            s.iterate(1)

    out, n = fresh_and_grown(make, start, grow, lambda s: split_phases(s, (2, 4, 2, 1)), "kept roll-out planes")
    assert n["k_search[stage 1]"] == 4 * ITERATIONS and n["k_search[stage 2]"] == 4 * ITERATIONS
    assert n["k_rollout[search]"] == 0 and n["k_rollout[stage 2 | winner]"] == 0
    assert np.all(np.isfinite(out[-1]["cost"]))


# ---------------------------------------------------------------------------
# 3. the per-trajectory table
# ---------------------------------------------------------------------------
def test_per_trajectory_table_grows_and_reads_back(ilqg):
    """set_params_batch with one size-1 name, then with every fixed-size name (W = 20), then with the one name again; init and
    two iterations behind each; params_batch(name) reads back what was set at every stage (a name that is not in the set reads
    the shared value).  Both forms of a kernel share its timing slot: the launch counts show the iterations, the read-back
    that the rows are the table's."""
    make, x0, u0 = car(ilqg)
    fixed = [n for n in CAR_PARAMS]
    assert sum(np.size(CAR_PARAMS[n]) for n in fixed) == 20
    table = {n: np.ascontiguousarray(t[:, 1]) for n, t in draws(CAR_PARAMS, fixed, B, 2).items()}
    assert limits_ordered({n: t[:, None] for n, t in table.items()})
    one = {"d": table["d"]}

    def start(s):
        s.set_params_batch(None)
        s.init(x0, u0)

    def grow(s):
        s.set_params_batch(table)
        s.init(x0, u0)
        s.iterate(1)

    def scenario(s):
        out = []
        for rows in (one, table, one):
            s.set_params_batch(rows)
            for n in fixed:
                want = rows[n] if n in rows else np.broadcast_to(np.asarray(CAR_PARAMS[n], dtype=np.float64), (B, np.size(CAR_PARAMS[n])))
                assert np.array_equal(s.params_batch(n), np.asarray(want).reshape(B, -1)), "params_batch(%s) with %d names" % (n, len(rows))
            s.init(x0, u0)
            s.iterate(ITERATIONS)
            out.append(snap(s))
        return out

    out, n = fresh_and_grown(make, start, grow, scenario, "per-trajectory table")
    assert n["k_backward[fused derivs]"] == 3 * ITERATIONS and n["k_search[stage 1]"] == 3 * ITERATIONS
    assert not np.array_equal(out[0]["cost"], out[1]["cost"])


# ---------------------------------------------------------------------------
# 4. the window futures and the log
# ---------------------------------------------------------------------------
def test_window_futures_and_the_log_grow_in_both_forms(ilqg):
    """receding(2 rounds of 1 step), then receding(5 rounds of 2 steps) on the same solver, one iteration a round: the log is made
    anew, the shared future [rounds * steps] grows; then `vref` gets rows per trajectory and the same two calls make the
    [B][rounds * steps] form grow."""
    make, x0, u0, vref, tracks, params = almix(ilqg)
    calls = ((2, 1), (5, 2))

    def start(s):
        s.set_param_steps_batch("vref", None)
        s.set_param("vref", vref[:N + 1])
        s.init(x0, u0)

    def grow(s):
        s.set_param_steps_batch("vref", tracks[:, :N + 1])
        s.init(x0, u0)
        s.receding(5, 2, 1, windows={"vref": tracks[:, N + 1:N + 11]})

    def scenario(s):
        out = []
        for rows in (False, True):
            if rows:
                s.set_param_steps_batch("vref", tracks[:, :N + 1])
                s.init(x0, u0)
            at = N + 1
            for rounds, steps in calls:
                future = tracks[:, at:at + rounds * steps] if rows else vref[at:at + rounds * steps]
                out.append(s.receding(rounds, steps, 1, windows={"vref": np.ascontiguousarray(future)}))
                at += rounds * steps
                out.append(dict(snap(s), window=s.param_steps_batch("vref")))
        return out

    out, n = fresh_and_grown(make, start, grow, scenario, "window futures and the log")
    rounds = 2 * sum(r for r, _ in calls)
    assert n["k_shift_windows"] == rounds and n["k_log_steps"] == rounds
    assert out[0]["x"].shape == (B, 2, 3) and out[2]["x"].shape == (B, 10, 3)
    assert np.array_equal(out[7]["window"], tracks[:, 12:12 + N + 1])  # 2 x 1 + 5 x 2 values on


# ---------------------------------------------------------------------------
# 5. the plants
# ---------------------------------------------------------------------------
def test_plants_are_made_anew_and_nothing_of_a_call_survives(ilqg):
    """receding_plant with two rounds and nothing named; on the same solver four rounds with a named parameter table and a
    disturbance; then, from the same start again, two rounds without them.  The third call equals the FRESH solver's first:
    nothing of the second call's table or disturbance survives."""
    make, x0, u0, vref, tracks, params = almix(ilqg)
    named = {n: np.ascontiguousarray(t[:, 1]) for n, t in draws(params, NAMED["almix"], B, 2).items()}
    dist = 0.01 * np.random.default_rng(62).standard_normal((B, 4 * 2, 3))

    def start(s):
        s.set_param("vref", vref[:N + 1])
        s.init(x0, u0)

    def grow(s):
        s.init(x0, u0)
        s.receding_plant(4, 2, 1, True, None, named, dist, windows={})

    def scenario(s):
        out = [s.receding_plant(2, 2, 1, True, None, None, None, windows={}), snap(s)]
        out += [s.receding_plant(4, 2, 1, True, None, named, dist, windows={}), snap(s)]
        start(s)
        out += [s.receding_plant(2, 2, 1, True, None, None, None, windows={}), snap(s)]
        return out

    out, n = fresh_and_grown(make, start, grow, scenario, "plants")
    assert n["k_plant"] == 2 + 4 + 2 and n["k_shift_windows"] == 2 + 4 + 2
    same(out[4:6], out[0:2], "the third call against the fresh solver's first")
    assert np.all(out[0]["ok"] == 1) and np.all(out[2]["ok"] == 1)


# ---------------------------------------------------------------------------
# 6. the wave mapping's kept roll-outs
# ---------------------------------------------------------------------------
def test_wave_mapping_candidates_of_both_stages_grow(ilqg):
    """synth16x8 FULL_DDP 1, B = 3, N = 6, ls_keep = 2: ls_split = 4, then 2 (the second stage's candidates grow from four step
    sizes to six), then 6 (the first stage's from four to six).  The path that keeps both stages' roll-outs ends every search
    with k_adopt and k_adopt_first in the winner's timing slot — two launches an iteration; the other paths have one."""
    b, n_hor = 3, 6
    x0, u0 = syn_inputs(b, n_hor)

    def make():
        return ilqg.BatchSolver("synth16x8", 1, batch=b, n_hor=n_hor, params=SYN_PARAMS_TIGHT, opts=dict(max_iter=40, ls_keep=2))

    def start(s):
        s.set_option("ls_split", 4)
        s.init(x0, u0)

    def grow(s):
        s.init(x0, u0)
        for split in (2, 6):
            s.set_option("ls_split", split)
            s.iterate(1)

    out, n = fresh_and_grown(make, start, grow, lambda s: split_phases(s, (4, 2, 6)), "wave mapping, kept roll-outs")
    assert n["k_rollout[winner]"] == 2 * 3 * ITERATIONS, "this library does not keep both stages' roll-outs (no k_adopt_first)"
    assert n["k_rollout[search]"] == 3 * ITERATIONS and n["k_rollout[stage 2 | winner]"] == 3 * ITERATIONS
    assert np.all(np.isfinite(out[-1]["cost"]))
