"""BatchSolver.policy_rollout(disturbance=...) on the GPU: every plan's policy rolled out under process noise, a push on the
state behind every step (k_policy with a disturbance table; ilqg_batch_policy_rollout_noise and its device and multi forms).

    x_{k+1} <- x_next + w[b][r][k]      k = 0 .. N-1        (w [B,R,N,nx], or [R,N,nx] for every trajectory)

Test 1 holds cost, ok, x, u and x_end of every compared slot and roll-out against the reference's own forward_pass taken one
step at a time through the CPU oracle's driver (policy_noise_cases.reference_disturbed_rollout, which
tests/test_policy_noise_recipe.py pins to one whole forward_pass and to the reference build) with the single-pass bar of
tests/test_gpu_policy_rollout.py, |d| <= 1e-10 max(1, |ref|).  The tables held to the reference have a ZERO LAST ROW: the
reference has no way to evaluate its final cost at a state it did not reach itself; what row N - 1 does is test 3's, by
identities.  The other tests are identities between calls of the product, bit for bit.  Builds, B = 70, SLOTS, R = 5, the
histories and the starts (r = 0: the plan's own x_0) are those of tests/test_gpu_policy_rollout.py; the noise is 0.01 N(0, I),
seeded, roll-out r = 0 of every trajectory under a zero table."""
import ctypes as C

import numpy as np
import pytest

import test_gpu_receding as base
from oracle.harness import lib_path
from params_batch_cases import dict_of, rows
from policy_cases import perturbed_starts
from policy_noise_cases import KINDS, R, reference_disturbed_rollout, step_params, tables, worst
from policy_param_cases import NAMED, SCALE, draws, limits_ordered, params_of
from test_gpu_policy_rollout import B, BUILDS, SLOTS, Case, ilqg, outputs_equal, to_numpy, torch  # noqa: F401

pytestmark = pytest.mark.gpu
close, state, assert_state_equal = base.close, base.state, base.assert_state_equal
KEYS = ("cost", "ok", "x_end", "x", "u")


def launches(s):
    t = s.kernel_times()
    return t["k_policy"][0] + t["k_policy_params"][0]


def held_to_the_reference(c, s, W, starts, params_at, label, **call):
    """every compared slot, kind and roll-out of s.policy_rollout(starts, disturbance=W, **call) against the chain under
    params_at(b, r); prints the worst deviation per output"""
    outs = [s.policy_rollout(starts, alpha, bool(feedback), trajectories=True, disturbance=W, **call) for alpha, feedback in KINDS]  # (before any getter)
    h = s.head(c.N, gains=True)
    cost = s.scalar("cost")
    mul = sum(s.multiplier_dims()) > 0
    w_l, w_f = (s.scalar("w_pen_l"), s.scalar("w_pen_f")) if mul else (np.zeros(B), np.zeros(B))
    m_run, m_fin = s.multipliers() if mul else (None, None)
    oracle = lib_path("oracle", c.problem, c.fd)
    moving = step_params(oracle, c.N)
    dev = dict(cost=0.0, x=0.0, u=0.0, x_end=0.0)
    for (alpha, feedback), out in zip(KINDS, outs):
        assert out["x"].shape == (B, R, c.N + 1, c.nx) and out["u"].shape == (B, R, c.N, c.nu) and out["ok"].dtype == np.int32
        for b in SLOTS:
            policy = (h["x"][b], h["u"][b], h["l"][b], h["L"][b])
            for r in range(R):
                ok, cr, xr, ur, _ = reference_disturbed_rollout(oracle, c.N, params_at(b, r), c.opts, starts[b, r], policy, alpha, feedback, w=W[b, r],
                                                                cost=cost[b], w_pen=(w_l[b], w_f[b]), multipliers=(m_run[b], m_fin[b]) if mul else None,
                                                                moving=moving)
                what = "%s alpha=%g feedback=%d slot %d roll-out %d" % (label, alpha, feedback, b, r)
                assert ok == 1, what + ": the oracle's roll-out is not finite (a compared roll-out may not be left out)"
                got = dict(cost=out["cost"][b, r], x=out["x"][b, r], u=out["u"][b, r], x_end=out["x_end"][b, r])
                want = dict(cost=cr, x=xr, u=ur, x_end=xr[-1])
                for k in got:
                    dev[k] = max(dev[k], worst(got[k], want[k]))
                assert out["ok"][b, r] == ok, what
                for k in got:
                    assert close(got[k], want[k]), "%s: %s off by %.3g" % (what, k, worst(got[k], want[k]))
    print("%s: worst deviation from the oracle's disturbed forward_pass " % label + ", ".join("%s %.3g" % kv for kv in dev.items()))


# ---------------------------------------------------------------------------
# 1. against the reference's forward_pass, one step at a time
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["fresh", "mid"])
@pytest.mark.parametrize("name,groups", BUILDS)
def test_disturbed_rollouts_equal_the_references_forward_pass(ilqg, name, groups, kind):
    c = Case(ilqg, name, groups)
    (s,) = c.history(kind)
    starts = perturbed_starts(c.x0, R, seed=17)
    held_to_the_reference(c, s, tables(c), starts, lambda b, r: c.params, "%s groups=%d %s" % (name, groups, kind))
    c.close()


@pytest.mark.parametrize("name", ["carparking", "synth16x8"])
def test_disturbed_rollouts_under_their_own_parameters_equal_the_reference(ilqg, name):
    """with a parameter table too (k_policy<true>): roll-out (b, r) under its own dict AND its own disturbance"""
    c = Case(ilqg, name, 0)
    (s,) = c.history("mid")
    table = draws(c.params, NAMED[name], B, R, scale=SCALE[name])
    assert limits_ordered(table)
    held_to_the_reference(c, s, tables(c, seed=5), perturbed_starts(c.x0, R, seed=17), lambda b, r: params_of(c.params, table, b, r),
                          "%s mid, a parameter table" % name, params=table)
    c.close()


def test_disturbed_rollouts_under_per_trajectory_rows_equal_the_reference(ilqg):
    """under per-trajectory rows (set_params_batch): trajectory b plans, and its roll-outs run, under b's row; with a table of
    the roll-outs' own on top the order is the trajectory's row, then the roll-out's"""
    c = Case(ilqg, "carparking", 0)
    (s,) = c.solvers
    table, mine = rows("carparking", c.params)
    s.set_params_batch(mine)
    c.history("mid")
    starts = perturbed_starts(c.x0, R, seed=17)
    held_to_the_reference(c, s, tables(c, seed=7), starts, lambda b, r: dict_of(c.params, table, b), "carparking mid, per-trajectory rows")
    own = draws(c.params, ("d", "cx"), B, R, seed=59, scale=SCALE["carparking"])
    held_to_the_reference(c, s, tables(c, seed=7), starts, lambda b, r: params_of(dict_of(c.params, table, b), own, b, r),
                          "carparking mid, per-trajectory rows and a parameter table", params=own)
    c.close()


# ---------------------------------------------------------------------------
# 2. identities
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("name,groups", BUILDS)
def test_no_table_a_zero_table_and_the_shared_table(ilqg, torch, name, groups):
    """the new entry with disturbance = NULL is the old entry bit for bit (and launches what it launches); a zero table gives
    equal values; a [R,N,nx] table is its expansion to [B,R,N,nx]; host form = device form; nothing of the batch changes"""
    c = Case(ilqg, name, groups, count=2)
    a, twin = c.history("mid")
    S = perturbed_starts(c.x0, R, seed=23)
    old = a.policy_rollout(S, alpha=0.25, trajectories=True)
    assert np.all(old["ok"] == 1)
    out = {k: np.full_like(old[k], -1) for k in KEYS}
    ptr = [out[k].ctypes.data_as(C.c_void_p) for k in KEYS]
    a.timing(True)
    n0 = launches(a)
    a._ck(a.lib.ilqg_batch_policy_rollout_noise(a.h, R, S.ctypes.data_as(C.c_void_p), 0, None, None, 0, None, 0, 0.25, 1, *ptr))
    assert launches(a) == n0 + a.groups() and a.kernel_times()["k_policy_params"][0] == 0
    a.timing(False)
    outputs_equal(out, old, "%s: the new entry without a table against the old entry" % name)
    zero = a.policy_rollout(S, alpha=0.25, trajectories=True, disturbance=np.zeros((B, R, c.N, c.nx)))
    outputs_equal(zero, old, "%s: a zero table" % name)
    Ws = tables(c, shared=True, last_zero=False)
    shared = a.policy_rollout(S, alpha=0.25, trajectories=True, disturbance=Ws)
    full = a.policy_rollout(S, alpha=0.25, trajectories=True, disturbance=np.ascontiguousarray(np.broadcast_to(Ws, (B,) + Ws.shape)))
    outputs_equal(shared, full, "%s: the shared table against its expansion" % name)
    assert not np.array_equal(shared["cost"][:, 1:], old["cost"][:, 1:]) and np.array_equal(shared["cost"][:, 0], old["cost"][:, 0])
    outputs_equal(a.policy_rollout(S, alpha=0.25, disturbance=Ws), shared, "%s: costs only" % name, ("cost", "ok", "x_end"))
    # device form: tables and starts written by work only enqueued on a side stream
    W = tables(c, last_zero=False)
    host = a.policy_rollout(S, alpha=0.25, trajectories=True, disturbance=W)
    torch.cuda.synchronize()
    s1 = torch.cuda.Stream()
    with torch.cuda.stream(s1):
        x0_t, w_t, ws_t = (torch.from_numpy(v).to("cuda", non_blocking=False) for v in (S, W, Ws))
        d = {k: v.clone() for k, v in a.policy_rollout(x0_t, alpha=0.25, trajectories=True, device=True, disturbance=w_t).items()}
        ds = {k: v.clone() for k, v in a.policy_rollout(x0_t, alpha=0.25, trajectories=True, device=True, disturbance=ws_t).items()}
        dn = {k: v.clone() for k, v in a.policy_rollout(x0_t, alpha=0.25, trajectories=True, device=True).items()}
    s1.synchronize()
    outputs_equal(to_numpy(d), host, "%s: device form against host form" % name)
    outputs_equal(to_numpy(ds), shared, "%s: device form, shared table" % name)
    outputs_equal(to_numpy(dn), old, "%s: device form without a table" % name)
    a.iterate(3)
    twin.iterate(3)
    assert_state_equal(state(a), state(twin), "%s: three iterations behind the disturbed roll-outs" % name)
    c.close()


@pytest.mark.parametrize("name,groups", BUILDS)
def test_bits_depend_on_slot_start_and_table_alone(ilqg, name, groups):
    """the bits of roll-out (b, r) do not depend on R or on the order along r"""
    c = Case(ilqg, name, groups)
    (s,) = c.history("mid")
    n = 70
    S = perturbed_starts(c.x0, n, seed=23)
    W = tables(c, n_starts=n, seed=11, last_zero=False)
    keys = ("cost", "ok", "x_end")
    full = s.policy_rollout(S, disturbance=W)
    assert np.all(full["ok"] == 1)
    whole = s.policy_rollout(S[:, :R], trajectories=True, disturbance=W[:, :R])
    outputs_equal(whole, {k: full[k][:, :R] for k in keys}, "R = 5 with whole roll-outs against R = 70", keys)
    assert np.array_equal(whole["x_end"], whole["x"][:, :, -1]) and np.array_equal(whole["x"][:, :, 0], S[:, :R])
    for r in (0, 3, 69):
        one = s.policy_rollout(S[:, r:r + 1], disturbance=W[:, r:r + 1])
        outputs_equal(one, {k: full[k][:, r:r + 1] for k in keys}, "roll-out %d alone against R = 70" % r)
    perm = np.random.default_rng(4).permutation(n)
    outputs_equal(s.policy_rollout(S[:, perm], disturbance=W[:, perm]), {k: full[k][:, perm] for k in keys}, "permuted along r")
    outputs_equal(s.policy_rollout(S[:, perm], disturbance=W[0][perm]), s.policy_rollout(S[:, perm], disturbance=np.broadcast_to(W[0][perm], W.shape)),
                  "permuted, shared table")
    c.close()


def test_groups_and_shards_give_the_same_bits(ilqg):
    """stream groups 0 / 2 / 4 of one batch, and ilqg_multi_policy_rollout_noise over three loop-back shards (a full table
    sharded by rows, a shared one given to every shard), with and without a parameter table.  B = 200 as in
    tests/test_gpu_policy_rollout.py: four groups need more than three tiles."""
    n = 200
    cases = [Case(ilqg, "carparking", g, batch=n) for g in (0, 2, 4)]
    c = cases[0]
    S = perturbed_starts(c.x0, R, seed=29)
    W = tables(c, seed=13, last_zero=False)
    assert W.shape == (n, R, c.N, c.nx)
    table = draws(c.params, NAMED["carparking"], n, R, scale=SCALE["carparking"])
    outs = []
    for q in cases:
        (s,) = q.history("mid")
        outs.append((s.policy_rollout(S, alpha=0.25, trajectories=True, disturbance=W), s.policy_rollout(S, disturbance=W[3]),
                     s.policy_rollout(S, trajectories=True, disturbance=W, params=table)))
    for g, o in zip((2, 4), outs[1:]):
        for mine, first in zip(o, outs[0]):
            outputs_equal(mine, first, "groups = %d against groups = 0" % g)
    m = ilqg.MultiSolver("carparking", 0, batch=n, n_hor=c.N, devices=[0] * 3, params=c.params, opts=dict(max_iter=40))
    m.init(c.x0, c.u0)
    m.iterate(7)
    outputs_equal(m.policy_rollout(S, alpha=0.25, trajectories=True, disturbance=W), outs[0][0], "three shards against the single batch")
    outputs_equal(m.policy_rollout(S, disturbance=W[3]), outs[0][1], "three shards, a shared table")
    outputs_equal(m.policy_rollout(S, trajectories=True, disturbance=W, params=table), outs[0][2], "three shards, a parameter table too")
    with pytest.raises(ilqg.IlqgError) as e:
        m._ck(m.lib.ilqg_multi_policy_rollout_noise(m.h, 0, S.ctypes.data_as(C.c_void_p), 0, None, None, 0, W.ctypes.data_as(C.c_void_p), 0, 1.0, 1,
                                                    None, None, None, None, None))
    assert "n_starts" in str(e.value)
    m.close()
    for q in cases:
        q.close()


# ---------------------------------------------------------------------------
# 3. the last row
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("name,groups", BUILDS)
def test_the_last_row_moves_the_end_state_and_nothing_before_it(ilqg, name, groups):
    """NOT held to the reference (it has no final cost at a state it did not reach itself); by identities instead.  With row
    N - 1 non-zero every output up to step N - 1 — u, x[:N] — has the bits of the run with that row zeroed, x_end is that run's
    x_end + w[N-1] (one addition, exactly), x[N] is x_end, and the cost — its final term is evaluated at the moved state —
    differs."""
    c = Case(ilqg, name, groups)
    (s,) = c.history("mid")
    S = perturbed_starts(c.x0, R, seed=31)
    W = tables(c, seed=17, last_zero=False)
    W[:, 0, -1] = 0.01  # (roll-out 0: a zero table but for the last row)
    Z = W.copy()
    Z[:, :, -1] = 0.0
    for alpha, feedback in KINDS:
        moved = s.policy_rollout(S, alpha, bool(feedback), trajectories=True, disturbance=W)
        still = s.policy_rollout(S, alpha, bool(feedback), trajectories=True, disturbance=Z)
        assert np.all(moved["ok"] == 1) and np.all(still["ok"] == 1)
        assert np.array_equal(moved["u"], still["u"]) and np.array_equal(moved["x"][:, :, :-1], still["x"][:, :, :-1])
        assert np.array_equal(moved["x_end"], still["x_end"] + W[:, :, -1]) and np.array_equal(moved["x"][:, :, -1], moved["x_end"])
        assert np.all(moved["cost"] != still["cost"])
    c.close()


# ---------------------------------------------------------------------------
# 4. k_policy and k_plant on each other
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("name,strict", [("carparking", True), ("carparking", None), ("synth16x8", None)])
def test_the_rollout_is_the_plant_of_the_closed_loop(ilqg, name, strict):
    """Behind iterate(3), R = 1, start = the plan's x_0 (the plants start there too), alpha = 0: the first `steps` steps of the disturbed roll-out are what
    receding_plant(rounds = 1, steps, iterations = 0, disturbance = w[:, :steps]) logs for its plants on an identical second
    solver, and the state behind step `steps` is the plant's final state — bit for bit in the FMA-free CarParking build (one
    text of the step in both kernels), at 1e-10 in the product builds."""
    steps = 4
    c = Case(ilqg, name, 0, count=2, strict=strict)
    a, b = c.solvers
    for s in (a, b):
        s.init(c.x0, c.u0)
        s.iterate(3)
    W = np.ascontiguousarray(tables(c, n_starts=2, seed=19, last_zero=False)[:, 1:])  # (tables() gives roll-out 0 a zero table)
    for feedback in (True, False):
        out = a.policy_rollout(c.x0[:, None, :], alpha=0.0, feedback=feedback, trajectories=True, disturbance=W)
        assert np.all(out["ok"] == 1)
        if feedback:  # (the loop shifts the plans: the second call would see another plan, so the twin runs it once per solver)
            p = b.receding_plant(1, steps, 0, feedback=True, x_plant=c.x0, disturbance=np.ascontiguousarray(W[:, 0, :steps]))
        else:
            p = a.receding_plant(1, steps, 0, feedback=False, x_plant=c.x0, disturbance=np.ascontiguousarray(W[:, 0, :steps]))
        assert np.all(p["ok"] == 1)
        got = (out["x"][:, 0, :steps], out["u"][:, 0, :steps], out["x"][:, 0, steps])
        want = (p["x"], p["u"], p["x_plant"])
        print("%s strict=%s feedback=%d: worst deviation x %.3g, u %.3g, the state behind step %d %.3g" % (
            name, strict, feedback, worst(got[0], want[0]), worst(got[1], want[1]), steps, worst(got[2], want[2])))
        for g, w_ in zip(got, want):
            assert np.array_equal(g, w_) if strict else close(g, w_)
    c.close()


# ---------------------------------------------------------------------------
# 5. failure is per roll-out
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("name,problem", [("carparking", None), ("synth16x8", None), ("synth16x8", "synth16x8_plain")])
def test_failure_is_per_rollout(ilqg, name, problem):
    """a NaN in one row of one roll-out's table, (64, 2) at step 3, and an Inf in a LAST row, (5, 1): ok = 0 for that roll-out
    alone — the disturbed state is tested as k_plant tests it, the state behind row N - 1 included — and every other roll-out
    has the bits of the clean run.  Both are data, not faults."""
    c = Case(ilqg, name, 0, problem=problem)
    (s,) = c.history("mid")
    S = perturbed_starts(c.x0, R, seed=37)
    W = tables(c, seed=23, last_zero=False)
    clean = s.policy_rollout(S, trajectories=True, disturbance=W)
    assert np.all(clean["ok"] == 1)
    bad_w = W.copy()
    bad_w[64, 2, 3, 1] = np.nan
    bad_w[5, 1, -1, 0] = np.inf
    bad = s.policy_rollout(S, trajectories=True, disturbance=bad_w)
    assert bad["ok"][64, 2] == 0 and bad["ok"][5, 1] == 0
    keep = np.ones((B, R), dtype=bool)
    keep[64, 2] = keep[5, 1] = False
    assert np.all(bad["ok"][keep] == 1)
    for k in clean:
        assert np.array_equal(bad[k][keep], clean[k][keep]), k
    # up to the step behind which the state was lost, the failed roll-outs are the clean ones too
    assert np.array_equal(bad["x"][64, 2, :4], clean["x"][64, 2, :4]) and np.array_equal(bad["u"][5, 1], clean["u"][5, 1])
    costs = s.policy_rollout(S, disturbance=bad_w)
    assert np.array_equal(costs["ok"], bad["ok"]) and np.array_equal(costs["cost"][keep], clean["cost"][keep])
    c.close()


# ---------------------------------------------------------------------------
# 6. refusals
# ---------------------------------------------------------------------------
def test_refused_calls_name_the_argument_and_launch_nothing(ilqg, torch):
    c = Case(ilqg, "almix", 0, count=2)
    a, b = c.history("mid")
    n = 3
    S = perturbed_starts(c.x0, n, seed=41)
    W = tables(c, n_starts=n)
    values = np.ones((B, n, 2))
    cost = np.zeros((B, n))
    good_x, good_w = torch.from_numpy(S).cuda(), torch.from_numpy(W).cuda()
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream or None)
    p = lambda v: v.ctypes.data_as(C.c_void_p)  # noqa: E731
    t = lambda v: C.c_void_p(v.data_ptr())  # noqa: E731
    names = lambda *s: (C.c_char_p * len(s))(*s)  # noqa: E731
    host, device = a.lib.ilqg_batch_policy_rollout_noise, a.lib.ilqg_batch_policy_rollout_noise_device
    a.timing(True)
    n0 = launches(a)

    def refused(call, *words):
        with pytest.raises(ilqg.IlqgError) as e:
            a._ck(call())
        for w in words:
            assert w in str(e.value), (w, str(e.value))

    # the parameter-name refusals of policy_rollout_params, through the new entry
    refused(lambda: host(a.h, n, p(S), 1, names(b"nosuch"), p(values), 0, p(W), 0, 1.0, 1, p(cost), None, None, None, None), "names[0]", "nosuch", "_noise")
    refused(lambda: host(a.h, n, p(S), 1, names(b"vref"), p(values), 0, p(W), 0, 1.0, 1, p(cost), None, None, None, None), "names[0]", "vref", "time step")
    refused(lambda: host(a.h, n, p(S), 2, names(b"lim", b"lim"), p(values), 0, p(W), 0, 1.0, 1, p(cost), None, None, None, None), "names[1]", "twice")
    refused(lambda: host(a.h, n, p(S), -1, names(b"lim"), p(values), 0, p(W), 0, 1.0, 1, p(cost), None, None, None, None), "n_names")
    refused(lambda: host(a.h, n, p(S), 1, None, p(values), 0, p(W), 0, 1.0, 1, p(cost), None, None, None, None), "names")
    refused(lambda: host(a.h, n, p(S), 1, names(b"lim"), None, 0, p(W), 0, 1.0, 1, p(cost), None, None, None, None), "values")
    # host memory given to the device form
    refused(lambda: device(a.h, n, t(good_x), 0, None, None, 0, p(W), 0, 1.0, 1, None, None, None, None, None, stream), "disturbance", "device memory")
    refused(lambda: device(a.h, n, p(S), 0, None, None, 0, t(good_w), 0, 1.0, 1, None, None, None, None, None, stream), "x0", "device memory")
    for bad in (0, -1):
        refused(lambda: host(a.h, bad, p(S), 0, None, None, 0, p(W), 0, 1.0, 1, p(cost), None, None, None, None), "n_starts", "ilqg_batch_policy_rollout_noise")
        refused(lambda: device(a.h, bad, t(good_x), 0, None, None, 0, t(good_w), 0, 1.0, 1, None, None, None, None, None, stream), "n_starts", "_noise_device")
    refused(lambda: host(a.h, n, None, 0, None, None, 0, p(W), 0, 1.0, 1, p(cost), None, None, None, None), "x0")
    for call, words in ((lambda: a.policy_rollout(S, disturbance=W[:, :, :-1]), ("disturbance", "shape")),
                        (lambda: a.policy_rollout(S, disturbance=good_w), ("disturbance", "device=True")),
                        (lambda: a.policy_rollout(good_x, device=True, disturbance=W), ("disturbance", "host")),
                        (lambda: a.policy_rollout(good_x, device=True, disturbance=good_w.float()), ("disturbance", "float64")),
                        (lambda: a.policy_rollout(good_x, device=True, disturbance=torch.zeros((B, n, c.N, 2 * c.nx), dtype=torch.float64, device="cuda")[..., ::2]),
                         ("disturbance", "contiguous"))):
        with pytest.raises(ilqg.IlqgError) as e:
            call()
        assert all(w in str(e.value) for w in words), str(e.value)
    # all outputs NULL: nothing to do, after the checks
    assert host(a.h, n, p(S), 0, None, None, 0, p(W), 0, 1.0, 1, None, None, None, None, None) == 0
    assert device(a.h, n, t(good_x), 0, None, None, 0, t(good_w), 1, 1.0, 1, None, None, None, None, None, stream) == 0
    assert launches(a) == n0, "a refused call launched the roll-out"
    assert host(a.h, n, p(S), 0, None, None, 0, p(W), 0, 1.0, 1, p(cost), None, None, None, None) == 0 and launches(a) == n0 + a.groups()
    a.timing(False)
    a.iterate(2)
    b.iterate(2)
    assert_state_equal(state(a), state(b), "two iterations behind refused calls")
    c.close()
