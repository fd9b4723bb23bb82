"""BatchSolver.policy_rollout(params=...) on the GPU: every plan's feedback policy rolled out from perturbed starts, each
roll-out under problem parameters of its own (k_policy<true>, ilqg_batch_policy_rollout_params).

Roll-out (b, r) is the reference's forward_pass (iLQG_func.tem:121-185) from the caller's start about the policy of slot b
— planned under the batch's parameters — evaluated with the batch's fixed-size parameters in which the named ones are
replaced by row (b, r) of the caller's table.  Test 1 holds every output against the reference's own forward_pass through
the CPU oracle's driver under that roll-out's parameter dict (tests/policy_cases.py, tests/policy_param_cases.py; pinned to
the reference build by tests/test_policy_rollout_params_recipe.py) with the single-pass bar of tests/test_gpu_receding.py,
|d| <= 1e-10 max(1, |ref|).  Test 2 holds nominal rows against the plain roll-out; tests 3 to 5 are identities within the
new kernel and bit for bit.  Builds, inputs, B = 70, SLOTS and histories are those of tests/test_gpu_policy_rollout.py;
R = 5, so that a wavefront mixes several slots and several draws."""
import ctypes as C

import numpy as np
import pytest

from oracle.harness import lib_path
from policy_cases import perturbed_starts, reference_rollout
from policy_param_cases import NAMED, PER_STEP, R, SCALE, draws, limits_ordered, nominal_table, params_of, reference_ok_under, width
from test_gpu_policy_rollout import B, SLOTS, Case, assert_state_equal, close, ilqg, outputs_equal, state, to_numpy, torch, worst  # noqa: F401

pytestmark = pytest.mark.gpu

KINDS = [(1.0, 1), (0.0, 0), (0.0, 1), (0.25, 0)]
KEYS = ("cost", "ok", "x_end")


def table_of(c, r=R, seed=None):
    kw = {} if seed is None else dict(seed=seed)
    t = draws(c.params, NAMED[c.name], B, r, scale=SCALE[c.name], **kw)
    assert limits_ordered(t)
    return t


def cut(table, rows):
    return {n: np.ascontiguousarray(t[:, rows]) for n, t in table.items()}


# ---------------------------------------------------------------------------
# 1. against the reference's forward_pass under every roll-out's own parameters
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("name,kind,strict", [(n, "mid", None) for n in NAMED] + [("carparking", "fresh", None), ("synth16x8", "mid", True)])
def test_rollouts_equal_the_references_forward_pass_under_their_parameters(ilqg, name, kind, strict):
    """strict=True, n = 16 problem: the FMA-free build, whose k_policy<true> reads every fixed-size parameter from global
    memory (ILQG_POLICY_PARAMS_IN_MEMORY, k_policy.inc) — the lane's row for a named one, the context's buffers for the rest"""
    c = Case(ilqg, name, 0, strict=strict)
    (s,) = c.history(kind)
    starts = perturbed_starts(c.x0, R, seed=17)
    table = table_of(c)
    assert width(c.params, NAMED[name]) == sum(t.shape[-1] for t in table.values())
    outs = [s.policy_rollout(starts, alpha, bool(feedback), trajectories=True, params=table) for alpha, feedback in KINDS]  # (before any getter)
    h = s.head(c.N, gains=True)
    cost = s.scalar("cost")
    mul = sum(s.multiplier_dims()) > 0
    w_l, w_f = (s.scalar("w_pen_l"), s.scalar("w_pen_f")) if mul else (np.zeros(B), np.zeros(B))
    m_run, m_fin = s.multipliers() if mul else (None, None)
    oracle = lib_path("oracle", c.problem, c.fd)
    dev = dict(cost=0.0, x=0.0, u=0.0, x_end=0.0)
    for (alpha, feedback), out in zip(KINDS, outs):
        assert out["x"].shape == (B, R, c.N + 1, c.nx) and out["u"].shape == (B, R, c.N, c.nu) and out["ok"].dtype == np.int32
        for b in SLOTS:
            policy = (h["x"][b], h["u"][b], h["l"][b], h["L"][b])
            for r in range(R):
                ok, cr, xr, ur = reference_rollout(oracle, c.N, params_of(c.params, table, b, r), c.opts, starts[b, r], policy, alpha, feedback,
                                                   cost=cost[b], w_pen=(w_l[b], w_f[b]), multipliers=(m_run[b], m_fin[b]) if mul else None)
                what = "%s %s alpha=%g feedback=%d slot %d row %d" % (name, kind, alpha, feedback, b, r)
                assert ok == 1, what + ": the oracle's roll-out is not finite (a compared roll-out may not be left out)"
                got = dict(cost=out["cost"][b, r], x=out["x"][b, r], u=out["u"][b, r], x_end=out["x_end"][b, r])
                want = dict(cost=cr, x=xr, u=ur, x_end=xr[-1])
                for k in got:
                    dev[k] = max(dev[k], worst(got[k], want[k]))
                assert out["ok"][b, r] == ok, what
                for k in got:
                    assert close(got[k], want[k]), "%s: %s off by %.3g" % (what, k, worst(got[k], want[k]))
    print("%s %s strict=%s: worst deviation from the oracle's forward_pass " % (name, kind, strict) + ", ".join("%s %.3g" % kv for kv in dev.items()))
    c.close()


# ---------------------------------------------------------------------------
# 2. nominal values give the plain roll-out
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("name,strict", [(n, None) for n in NAMED] + [("carparking", True), ("synth16x8", True)])
def test_nominal_rows_give_the_plain_rollout(ilqg, name, strict):
    """bit for bit in the FMA-free builds: CarParking's k_policy<true> keeps the overridden parameters in registers, the
    n = 16 problem's reads all of them from global memory (k_policy.inc), and both must give the plain kernel's bits"""
    c = Case(ilqg, name, 0, strict=strict)
    (s,) = c.history("mid")
    starts = perturbed_starts(c.x0, R, seed=17)
    for alpha, feedback in ((1.0, True), (0.0, False)):
        plain = s.policy_rollout(starts, alpha, feedback, trajectories=True)
        named = s.policy_rollout(starts, alpha, feedback, trajectories=True, params=nominal_table(c.params, NAMED[name], B))
        assert np.all(plain["ok"] == 1) and np.array_equal(named["ok"], plain["ok"])
        print("%s strict=%s alpha=%g: worst deviation from the plain roll-out " % (name, strict, alpha) +
              ", ".join("%s %.3g" % (k, worst(named[k], plain[k])) for k in ("cost", "x", "u", "x_end")))
        if strict:
            outputs_equal(named, plain, "nominal rows against the plain roll-out, FMA-free build")
        else:
            for k in ("cost", "x", "u", "x_end"):
                assert close(named[k], plain[k]), k
    c.close()


# ---------------------------------------------------------------------------
# 3. a roll-out's bits depend on nothing but its slot, its start and its parameter row
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(NAMED))
def test_bits_depend_on_slot_start_and_row_alone(ilqg, torch, name):
    c = Case(ilqg, name, 0)
    (s,) = c.history("mid")
    names = NAMED[name]
    S = perturbed_starts(c.x0, 64, seed=23)
    T = table_of(c, 64, seed=59)
    full = s.policy_rollout(S, params=T)
    assert sorted(full) == sorted(KEYS)
    five = s.policy_rollout(S[:, :R], trajectories=True, params=cut(T, slice(0, R)))
    assert np.all(five["ok"] == 1)
    outputs_equal(five, {k: full[k][:, :R] for k in KEYS}, "R = 5 against R = 64", KEYS)
    assert np.array_equal(five["x_end"], five["x"][:, :, -1]) and np.array_equal(five["x"][:, :, 0], S[:, :R])
    perm = np.random.default_rng(4).permutation(64)
    outputs_equal(s.policy_rollout(S[:, perm], params=cut(T, perm)), {k: full[k][:, perm] for k in KEYS}, "starts and rows permuted along r")
    # one [R, W] table for every trajectory is its expansion to [B, R, W]
    one = {n: T[n][7, :R].copy() for n in names}
    shared = s.policy_rollout(S[:, :R], alpha=0.25, params=one)
    outputs_equal(shared, s.policy_rollout(S[:, :R], alpha=0.25, params={n: np.broadcast_to(t, (B,) + t.shape) for n, t in one.items()}), "[R, W] against [B, R, W]")
    assert not np.array_equal(shared["cost"], s.policy_rollout(S[:, :R], alpha=0.25)["cost"])  # (the table is no no-op)
    # an extra parameter named with the batch's own values
    extra = next(n for n, size in s.problem.params if size > 0 and n not in names)
    more = dict(cut(T, slice(0, R)), **nominal_table(c.params, (extra,), B))
    outputs_equal(s.policy_rollout(S[:, :R], trajectories=True, params=more), five, "%s named with nominal values" % extra)
    # the names in another order, the columns with them
    outputs_equal(s.policy_rollout(S[:, :R], trajectories=True, params={n: T[n][:, :R] for n in reversed(names)}), five, "names in reverse order")
    # device form, on a side stream of the caller, the table packed by torch.cat there; and a single tensor read where it is
    src = torch.from_numpy(S[:, :R].copy()).cuda()
    tens = {n: torch.from_numpy(np.ascontiguousarray(T[n][:, :R])).cuda() for n in names}
    torch.cuda.synchronize()
    s1 = torch.cuda.Stream()
    with torch.cuda.stream(s1):
        d = s.policy_rollout(src.clone(), trajectories=True, device=True, params={n: t.clone() for n, t in tens.items()})
        d = {k: v.clone() for k, v in d.items()}
    s1.synchronize()
    assert all(v.is_cuda for v in d.values()) and d["ok"].dtype == torch.int32
    outputs_equal(to_numpy(d), five, "device form against host form")
    first = names[0]
    outputs_equal(to_numpy(s.policy_rollout(src, device=True, params={first: tens[first]})), s.policy_rollout(S[:, :R], params={first: T[first][:, :R]}),
                  "device form, one tensor")
    dshared = s.policy_rollout(src, alpha=0.25, device=True, params={n: torch.from_numpy(t).cuda() for n, t in one.items()})
    outputs_equal(to_numpy(dshared), shared, "device form, [R, W]")
    c.close()


def test_groups_and_shards_give_the_same_bits(ilqg):
    """stream groups 1 and 2 of one batch, and ilqg_multi_policy_rollout_params over three shards (24, 24 and 22
    trajectories) on one device: the table is offset by the group's / the shard's first trajectory, unless it is shared"""
    cases = [Case(ilqg, "carparking", g) for g in (0, 1, 2)]
    c = cases[0]
    S = perturbed_starts(c.x0, R, seed=29)
    T = table_of(c, seed=61)
    one = {n: t[3].copy() for n, t in T.items()}
    outs, shared = [], []
    for q in cases:
        (s,) = q.history("mid")
        outs.append(s.policy_rollout(S, alpha=0.25, trajectories=True, params=T))
        shared.append(s.policy_rollout(S, params=one))
    for g, o, sh in zip((1, 2), outs[1:], shared[1:]):
        outputs_equal(o, outs[0], "groups = %d against the library's choice" % g)
        outputs_equal(sh, shared[0], "groups = %d, shared table" % g)
    m = ilqg.MultiSolver("carparking", 0, batch=B, n_hor=c.N, devices=[0] * 3, params=c.params, opts=dict(max_iter=40))
    m.init(c.x0, c.u0)
    m.iterate(7)
    outputs_equal(m.policy_rollout(S, alpha=0.25, trajectories=True, params=T), outs[0], "three shards against the single batch")
    outputs_equal(m.policy_rollout(S, params=one), shared[0], "three shards, shared table")
    m.close()
    for q in cases:
        q.close()


# ---------------------------------------------------------------------------
# 4. no side effects
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["carparking", "synth16x8", "almix"])
def test_rollouts_under_other_parameters_change_nothing_in_the_batch(ilqg, name):
    c = Case(ilqg, name, 0, count=2)
    a, b = c.history("mid")
    S = perturbed_starts(c.x0, R, seed=19)
    T = table_of(c)
    a.policy_rollout(S, trajectories=True, params=T)
    a.policy_rollout(S, alpha=0.0, feedback=False, params={n: t[0] for n, t in T.items()})
    assert_state_equal(state(a), state(b), "%s: state behind the roll-outs" % name)
    outputs_equal(a.policy_rollout(S, trajectories=True), b.policy_rollout(S, trajectories=True), "%s: the parameters a later plain roll-out sees" % name)
    a.iterate(3)
    b.iterate(3)
    assert_state_equal(state(a), state(b), "%s: three iterations behind the roll-outs" % name)
    c.close()


# ---------------------------------------------------------------------------
# 5. failure is per roll-out
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["carparking", "synth10hx"])
def test_failure_is_per_rollout(ilqg, name):
    """one row, (64, 2), whose time step h is NaN — data, not a fault: its ok is what the oracle's forward_pass returns
    under those parameters, every other roll-out of the call keeps its bits"""
    c = Case(ilqg, name, 0)
    (s,) = c.history("mid")
    names = NAMED[name] if "h" in NAMED[name] else NAMED[name] + ("h",)
    S = perturbed_starts(c.x0, R, seed=37)
    T = draws(c.params, names, B, R, scale=SCALE[name])
    clean = s.policy_rollout(S, trajectories=True, params=T)
    assert np.all(clean["ok"] == 1)
    bad_table = {n: t.copy() for n, t in T.items()}
    bad_table["h"][64, 2, 0] = np.nan
    bad = s.policy_rollout(S, trajectories=True, params=bad_table)
    h = s.head(c.N, gains=True)
    mul = sum(s.multiplier_dims()) > 0
    ok, _ = reference_ok_under(lib_path("oracle", c.problem, c.fd), c.N, c.params, {n: bad_table[n][64, 2] for n in names}, c.opts, S[64, 2],
                               (h["x"][64], h["u"][64], h["l"][64], h["L"][64]), 1.0, 1, cost=s.scalar("cost")[64],
                               w_pen=(s.scalar("w_pen_l")[64], s.scalar("w_pen_f")[64]) if mul else (0.0, 0.0),
                               multipliers=tuple(m[64] for m in s.multipliers()) if mul else None)
    print("%s: the oracle's forward_pass under h = NaN returns %d, the roll-out's ok is %d" % (name, ok, bad["ok"][64, 2]))
    assert bad["ok"][64, 2] == ok
    keep = np.ones((B, R), dtype=bool)
    keep[64, 2] = False
    assert np.all(bad["ok"][keep] == 1)
    for k in clean:
        assert np.array_equal(bad[k][keep], clean[k][keep]), k
    costs = s.policy_rollout(S, params=bad_table)
    assert np.array_equal(costs["ok"], bad["ok"]) and np.array_equal(costs["cost"][keep], clean["cost"][keep])
    c.close()


# ---------------------------------------------------------------------------
# 6. refusals
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["carparking", "almix"])
def test_refused_calls_name_the_argument_or_parameter_and_change_nothing(ilqg, torch, name):
    c = Case(ilqg, name, 2 if name == "carparking" else 0, count=2)
    a, b = c.history("mid")
    names = NAMED[name]
    S = perturbed_starts(c.x0, 3, seed=41)
    T = draws(c.params, names, B, 3)
    V = np.ascontiguousarray(np.concatenate([T[n] for n in names], axis=-1))
    S_dev, V_dev = torch.from_numpy(S).cuda(), torch.from_numpy(V).cuda()
    cost = np.full((B, 3), -7.0)
    cost_dev = torch.full((B, 3), -7.0, dtype=torch.float64, device="cuda")
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream or None)

    def strings(*words):
        return (C.c_char_p * max(len(words), 1))(*[w.encode() for w in words])

    def host(n_names, arr, values=V, n_starts=3, x0=S):
        return lambda: a._ck(a.lib.ilqg_batch_policy_rollout_params(a.h, n_starts, None if x0 is None else C.c_void_p(x0.ctypes.data), n_names, arr,
                                                                     None if values is None else C.c_void_p(values.ctypes.data), 0, 1.0, 1,
                                                                     C.c_void_p(cost.ctypes.data), None, None, None, None))

    def device(n_names, arr, values, x0=None):
        return lambda: a._ck(a.lib.ilqg_batch_policy_rollout_params_device(a.h, 3, C.c_void_p(S_dev.data_ptr()) if x0 is None else x0, n_names, arr, values, 0,
                                                                            1.0, 1, C.c_void_p(cost_dev.data_ptr()), None, None, None, None, stream))

    def refused(call, *words):
        with pytest.raises(ilqg.IlqgError) as e:
            call()
        for w in words:
            assert w in str(e.value), (w, str(e.value))

    good = strings(*names)
    dv = C.c_void_p(V_dev.data_ptr())
    for form, who in ((lambda n, arr: host(n, arr), "ilqg_batch_policy_rollout_params"), (lambda n, arr: device(n, arr, dv), "ilqg_batch_policy_rollout_params_device")):
        refused(form(len(names), strings(*(names[:-1] + ("nope",)))), who, "names", "Parameter name 'nope' is not member of parameters struct.")
        refused(form(len(names), strings(*(names[:-1] + (names[0],)))), who, "names", "'%s'" % names[0], "twice")
        refused(form(0, good), who, "n_names")
        refused(form(len(names), None), who, "names")
        if name in PER_STEP:
            refused(form(len(names), strings(*(names[:-1] + (PER_STEP[name],)))), who, "names", "'%s'" % PER_STEP[name], "per-time-step parameters stay shared")
    refused(host(len(names), good, values=None), "values")
    refused(host(len(names), good, n_starts=0), "n_starts")
    refused(host(len(names), good, x0=None), "x0")
    refused(device(len(names), good, None), "values")
    refused(device(len(names), good, C.c_void_p(V.ctypes.data)), "values", "device memory")      # host memory given to the device form
    refused(device(len(names), good, dv, x0=C.c_void_p(S.ctypes.data)), "x0", "device memory")
    refused(lambda: a.policy_rollout(S, params={names[0]: torch.from_numpy(T[names[0]]).cuda()}), "params", names[0], "device=True")
    refused(lambda: a.policy_rollout(S_dev, device=True, params={names[0]: T[names[0]]}), "params", names[0], "host")
    if name in PER_STEP:
        refused(lambda: a.policy_rollout(S, params={PER_STEP[name]: np.zeros((B, 3, c.N + 1))}), "params", PER_STEP[name], "stay shared")
    torch.cuda.synchronize()
    assert np.all(cost == -7.0) and bool(torch.all(cost_dev == -7.0)), "a refused call wrote an output"
    # all outputs NULL: nothing to do, after validation
    assert a.lib.ilqg_batch_policy_rollout_params(a.h, 3, C.c_void_p(S.ctypes.data), len(names), good, C.c_void_p(V.ctypes.data), 0, 1.0, 1, None, None, None, None, None) == 0
    assert a.lib.ilqg_batch_policy_rollout_params(a.h, 3, C.c_void_p(S.ctypes.data), 0, good, C.c_void_p(V.ctypes.data), 0, 1.0, 1, None, None, None, None, None) != 0
    assert a.lib.ilqg_batch_policy_rollout_params_device(a.h, 3, C.c_void_p(S_dev.data_ptr()), len(names), good, dv, 0, 1.0, 1, None, None, None, None, None, stream) == 0
    # and the good call through the raw entry gives what the method gives
    assert a.lib.ilqg_batch_policy_rollout_params(a.h, 3, C.c_void_p(S.ctypes.data), len(names), good, C.c_void_p(V.ctypes.data), 0, 1.0, 1, C.c_void_p(cost.ctypes.data),
                                                  None, None, None, None) == 0
    assert np.array_equal(cost, b.policy_rollout(S, params=T)["cost"])
    assert_state_equal(state(a), state(b), "state behind refused calls")
    a.iterate(2)
    b.iterate(2)
    assert_state_equal(state(a), state(b), "two iterations behind refused calls")
    c.close()
