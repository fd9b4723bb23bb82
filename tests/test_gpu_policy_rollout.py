"""BatchSolver.policy_rollout on the GPU: every plan's feedback policy rolled out from perturbed starts (k_policy).

The policy of a trajectory is what head(N, gains=True) returns for it; a roll-out is the reference's forward_pass
(iLQG_func.tem:121-185) from the caller's start about that policy, with u_k = u_nom_k [+ alpha l_k] [+ L_k (x_k - x_nom_k)].
Test 1 holds every output against the reference's own forward_pass through the CPU oracle's driver (the recipe of
tests/policy_cases.py, which tests/test_policy_rollout_recipe.py pins to the reference build) with the single-pass bar of
tests/test_gpu_parity.py, |d| <= 1e-10 max(1, |ref|); the other tests are identities between calls of the product and are
bit for bit.  Builds, inputs and histories are those of tests/test_gpu_receding.py with B = 70 (two tiles, a ragged last
one): "fresh" = init, calc_derivs, back_pass (the gains are about the plan itself), "mid" = init, iterate(7) (in
CarParking's lane mapping some current trajectories then live in kept roll-out planes of the line search, others in X / U;
behind an accepted step the gains are about the previous nominal trajectory).  Starts: r = 0 is the plan's own x_0 bit for
bit, the others x_0 + 0.1 N(0, I) (CPU oracle: every compared roll-out of every build and history is finite, ok = 1)."""
import ctypes as C
import os

import numpy as np
import pytest

import test_gpu_receding as base
from oracle.harness import lib_path
from policy_cases import COMBOS, perturbed_starts, reference_rollout

pytestmark = pytest.mark.gpu

BUILDS = [("carparking", 0), ("carparking", 2), ("carparking_wave", 0), ("hxtest", 0), ("synth16x8", 0), ("synth10hx", 0), ("almix", 0)]
B = 70
SLOTS = (0, 63, 64, 69)
close, state, assert_state_equal = base.close, base.state, base.assert_state_equal


@pytest.fixture(scope="module")
def ilqg():
    import __graft_entry__ as g
    g.load_package()
    from ddp_generator_amd import ilqg as m
    if not all(os.path.exists(m.library_path(p, fd, st)) for p, fd, st in
               (("carparking", 0, False), ("carparking", 0, "wave"), ("carparking", 0, True), ("hxtest", 1, False), ("synth16x8", 1, False),
                ("synth16x8_plain", 1, False), ("synth10hx", 0, False), ("almix", 1, False))):
        g.build_for_tests()
    if m.Problem("carparking", 0).device_count() < 1:
        pytest.fail("no HIP device visible: the GPU tests must run on the MI355X box")
    return m


@pytest.fixture(scope="module")
def torch():
    import torch as t
    assert t.cuda.is_available()
    return t


class Case:
    """`count` solvers of one build (tests/test_gpu_receding.py:setup) with the same history"""

    def __init__(self, ilqg, name, groups=0, count=1, strict=None, problem=None, batch=B):
        self.name = name
        prob, self.fd, st, self.N, self.params, self.opts, self.x0, self.u0 = base.setup(name, batch)
        self.problem = problem or prob
        kw = dict(batch=batch, n_hor=self.N, params=self.params, opts=dict(self.opts, max_iter=40), strict=st if strict is None else strict, groups=groups)
        self.solvers = [ilqg.BatchSolver(self.problem, self.fd, **kw) for _ in range(count)]
        if groups:
            assert self.solvers[0].groups() == groups
        self.nx, self.nu = self.solvers[0].problem.nx, self.solvers[0].problem.nu

    def history(self, kind):
        for s in self.solvers:
            s.init(self.x0, self.u0)
            if kind == "fresh":
                s.calc_derivs()
                s.back_pass()
            elif kind == "mid":
                s.iterate(7)
        if kind == "mid" and self.name == "carparking":
            # both locations occur (tests/test_gpu_mpc_loop.py): kept roll-out planes (ILQG_I_LOC != 0) and X / U — the case
            # a read of the nominal trajectory can get wrong.  (CPU oracle, reference build and its FMA build at B = 70:
            # one step accepted in the second stage, slot 61, the other 69 in the first.)
            acc, idx = self.solvers[0].ints("accepted"), self.solvers[0].ints("alpha_idx")
            assert np.any((acc == 1) & (idx <= 4)) and np.any((acc == 0) | (idx > 4))
        return self.solvers

    def close(self):
        for s in self.solvers:
            s.close()


def outputs_equal(a, b, what, keys=None):
    for k in keys or sorted(a):
        assert np.array_equal(np.asarray(a[k]), np.asarray(b[k])), "%s: %s differs" % (what, k)


def to_numpy(out):
    return {k: v.cpu().numpy() for k, v in out.items()}


def worst(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.max(np.abs(a - b) / np.maximum(1.0, np.abs(b)))) if a.size else 0.0


# ---------------------------------------------------------------------------
# 1. against the reference's forward_pass
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["fresh", "mid"])
@pytest.mark.parametrize("name,groups", BUILDS)
def test_rollouts_equal_the_references_forward_pass(ilqg, name, groups, kind):
    R = 5
    c = Case(ilqg, name, groups)
    (s,) = c.history(kind)
    starts = perturbed_starts(c.x0, R, seed=17)
    outs = [s.policy_rollout(starts, alpha, bool(feedback), trajectories=True) for alpha, feedback in COMBOS]  # (before any getter)
    h = s.head(c.N, gains=True)
    assert np.array_equal(h["x"][:, 0], c.x0) and np.array_equal(starts[:, 0], c.x0)
    cost = s.scalar("cost")
    mul = sum(s.multiplier_dims()) > 0
    w_l, w_f = (s.scalar("w_pen_l"), s.scalar("w_pen_f")) if mul else (np.zeros(B), np.zeros(B))
    m_run, m_fin = s.multipliers() if mul else (None, None)
    oracle = lib_path("oracle", c.problem, c.fd)
    dev = dict(cost=0.0, x=0.0, u=0.0, x_end=0.0)
    for (alpha, feedback), out in zip(COMBOS, outs):
        assert out["x"].shape == (B, R, c.N + 1, c.nx) and out["u"].shape == (B, R, c.N, c.nu) and out["ok"].dtype == np.int32
        for b in SLOTS:
            policy = (h["x"][b], h["u"][b], h["l"][b], h["L"][b])
            for r in range(R):
                ok, cr, xr, ur = reference_rollout(oracle, c.N, c.params, c.opts, starts[b, r], policy, alpha, feedback, cost=cost[b],
                                                   w_pen=(w_l[b], w_f[b]), multipliers=(m_run[b], m_fin[b]) if mul else None)
                what = "%s %s alpha=%g feedback=%d slot %d start %d" % (name, kind, alpha, feedback, b, r)
                assert ok == 1, what + ": the oracle's roll-out is not finite (a compared roll-out may not be left out)"
                got = dict(cost=out["cost"][b, r], x=out["x"][b, r], u=out["u"][b, r], x_end=out["x_end"][b, r])
                want = dict(cost=cr, x=xr, u=ur, x_end=xr[-1])
                for k in got:
                    dev[k] = max(dev[k], worst(got[k], want[k]))
                assert out["ok"][b, r] == ok, what
                for k in got:
                    assert close(got[k], want[k]), "%s: %s off by %.3g" % (what, k, worst(got[k], want[k]))
    print("%s groups=%d %s: worst deviation from the oracle's forward_pass " % (name, groups, kind) + ", ".join("%s %.3g" % kv for kv in dev.items()))
    c.close()


# ---------------------------------------------------------------------------
# 2. replay identity
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["init", "fresh"])
@pytest.mark.parametrize("name,groups,strict", [(n, g, None) for n, g in BUILDS] + [("carparking", 0, True)])
def test_open_loop_replay_from_the_plans_own_start_is_the_plan(ilqg, name, groups, strict, kind):
    """alpha = 0, feedback = 0, R = 1, start = the plan's x_0: x, u and the cost are the plan's — within the single-pass bar in
    the product builds (the roll-out that stored the plan is another kernel: other FMA contractions), bit for bit in the
    FMA-free CarParking build, where equal source order gives equal bits.  (almix: x and u only.  The cost its batch holds
    here is that of the initial roll-out, which runs with zero penalty weights, iLQG_mex.c:23,116, while policy_rollout
    uses the weights the trajectory has now; its cost is held against the oracle in test 1.)"""
    c = Case(ilqg, name, groups, strict=strict)
    (s,) = c.history(kind)
    out = s.policy_rollout(c.x0[:, None, :], alpha=0.0, feedback=False, trajectories=True)
    x, u, cost = s.x(), s.u(), s.scalar("cost")
    assert np.all(out["ok"] == 1)
    print("%s groups=%d strict=%s %s: worst deviation x %.3g, u %.3g, cost %.3g" % (name, groups, strict, kind, worst(out["x"][:, 0], x),
                                                                                 worst(out["u"][:, 0], u), worst(out["cost"][:, 0], cost)))
    if strict:
        assert np.array_equal(out["x"][:, 0], x) and np.array_equal(out["u"][:, 0], u) and np.array_equal(out["cost"][:, 0], cost)
    else:
        assert close(out["x"][:, 0], x) and close(out["u"][:, 0], u)
        if name != "almix":
            assert close(out["cost"][:, 0], cost)
    assert np.array_equal(out["x_end"], out["x"][:, :, -1])
    c.close()


# ---------------------------------------------------------------------------
# 3. a roll-out's bits depend on nothing but its slot and its start
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("name,groups", BUILDS)
def test_bits_depend_on_slot_and_start_alone(ilqg, torch, name, groups):
    """the same starts as R = 70 (B * R = 4 900 roll-outs), R = 64, R = 5, one at a time, permuted along r, costs only and
    with whole roll-outs, through the host form and through the device form on a side stream of the caller"""
    c = Case(ilqg, name, groups)
    (s,) = c.history("mid")
    S = perturbed_starts(c.x0, 70, seed=23)
    keys = ("cost", "ok", "x_end")
    full = s.policy_rollout(S)
    assert sorted(full) == sorted(keys) and np.all(full["ok"] == 1)
    part = s.policy_rollout(S[:, :64])
    outputs_equal(part, {k: full[k][:, :64] for k in keys}, "R = 64 against R = 70")
    whole = s.policy_rollout(S[:, :5], trajectories=True)
    outputs_equal(whole, {k: full[k][:, :5] for k in keys}, "R = 5 with whole roll-outs against R = 70", keys)
    assert np.array_equal(whole["x_end"], whole["x"][:, :, -1]) and np.array_equal(whole["x"][:, :, 0], S[:, :5])
    outputs_equal(s.policy_rollout(S[:, :5]), whole, "costs only against whole roll-outs", keys)
    for r in (0, 3, 69):
        one = s.policy_rollout(S[:, r:r + 1])
        outputs_equal(one, {k: full[k][:, r:r + 1] for k in keys}, "start %d alone against R = 70" % r)
    perm = np.random.default_rng(4).permutation(70)
    outputs_equal(s.policy_rollout(S[:, perm]), {k: full[k][:, perm] for k in keys}, "permuted along r")
    # [R, nx] for every trajectory is [B, R, nx] with equal rows
    shared = s.policy_rollout(S[7, :5], alpha=0.25, feedback=True)
    outputs_equal(shared, s.policy_rollout(np.broadcast_to(S[7, :5], (B, 5, c.nx)), alpha=0.25, feedback=True), "[R, nx] broadcast")
    # device form: the starts are written, and the outputs read, by work only ENQUEUED on a side stream; no host sync between
    src = torch.from_numpy(S[:, :5].copy()).cuda()
    x0_t = torch.zeros((B, 5, c.nx), dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    s1 = torch.cuda.Stream()
    with torch.cuda.stream(s1):
        x0_t.copy_(src)
        d = s.policy_rollout(x0_t, trajectories=True, device=True)
        d = {k: v.clone() for k, v in d.items()}
        dc = s.policy_rollout(x0_t, device=True)
        doubled = dc["cost"] * 2.0  # consumed on the caller's stream (an exact operation)
    s1.synchronize()
    assert all(v.is_cuda for v in d.values()) and d["ok"].dtype == torch.int32 and d["cost"].dtype == torch.float64
    outputs_equal(to_numpy(d), whole, "device form against host form")
    outputs_equal(to_numpy(dc), whole, "device form, costs only", keys)
    assert np.array_equal(doubled.cpu().numpy(), whole["cost"] * 2.0)
    # single outputs through the raw entry, every other pointer NULL
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream or None)
    xe = torch.full((B, 5, c.nx), np.nan, dtype=torch.float64, device="cuda")
    assert s.lib.ilqg_batch_policy_rollout_device(s.h, 5, C.c_void_p(src.data_ptr()), 1.0, 1, None, None, C.c_void_p(xe.data_ptr()), None, None, stream) == 0
    assert np.array_equal(xe.cpu().numpy(), whole["x_end"])
    c.close()


def test_groups_and_shards_give_the_same_bits(ilqg):
    """stream groups 0 / 2 / 4 of one batch, and ilqg_multi_policy_rollout over three shards on one device.  B = 200 here: a
    group is whole tiles of 64 trajectories, so four groups need more than three tiles (1 000 roll-outs)."""
    n = 200
    cases = [Case(ilqg, "carparking", g, batch=n) for g in (0, 2, 4)]
    S = perturbed_starts(cases[0].x0, 5, seed=29)
    outs = []
    for c in cases:
        (s,) = c.history("mid")
        outs.append(s.policy_rollout(S, alpha=0.25, trajectories=True))
    for g, o in zip((2, 4), outs[1:]):
        outputs_equal(o, outs[0], "groups = %d against groups = 0" % g)
    c = cases[0]
    m = ilqg.MultiSolver("carparking", 0, batch=n, n_hor=c.N, devices=[0] * 3, params=c.params, opts=dict(max_iter=40))
    m.init(c.x0, c.u0)
    m.iterate(7)
    outputs_equal(m.policy_rollout(S, alpha=0.25, trajectories=True), outs[0], "three shards against the single batch")
    outputs_equal(m.policy_rollout(S[0], alpha=0.0), c.solvers[0].policy_rollout(S[0], alpha=0.0), "three shards, [R, nx]")
    with pytest.raises(ilqg.IlqgError) as e:
        m.lib.ilqg_multi_policy_rollout.restype = C.c_int
        m._ck(m.lib.ilqg_multi_policy_rollout(m.h, 0, C.c_void_p(S.ctypes.data), 1.0, 1, None, None, None, None, None))
    assert "n_starts" in str(e.value)
    m.close()
    for c in cases:
        c.close()


# ---------------------------------------------------------------------------
# 4. no side effects
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("name,groups", BUILDS)
def test_rollouts_change_nothing_in_the_batch(ilqg, name, groups):
    c = Case(ilqg, name, groups, count=2)
    a, b = c.history("mid")
    S = perturbed_starts(c.x0, 5, seed=19)
    before = a.head(c.N, gains=True)
    a.policy_rollout(S, trajectories=True)
    a.policy_rollout(S, alpha=0.0, feedback=False)
    outputs_equal(a.head(c.N, gains=True), before, "%s: head behind the roll-outs" % name)
    a.iterate(3)
    b.iterate(3)
    assert_state_equal(state(a), state(b), "%s: three iterations behind the roll-outs" % name)
    c.close()


# ---------------------------------------------------------------------------
# 5. failure is per roll-out
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("name,problem", [("carparking", None), ("synth16x8", None), ("synth16x8", "synth16x8_plain")])
def test_failure_is_per_rollout(ilqg, name, problem):
    """One start with a NaN component, (64, 2), and one whose first component is 1e200, (5, 1): finite, but its square in the
    running cost is not (CPU oracle: forward_pass returns 0 at step 0 for both problems).  Their ok is 0; every other
    roll-out has the bits of the run without them.  The n = 16 builds have wave-uniform guards (tests/test_gpu_parity.py
    test_failure_paths_are_per_trajectory_with_uniform_guards): a failing lane makes its wavefront repeat the step lane by
    lane, in the same machine code; `_plain` is the pair whose callbacks work on the private element with proxies.
    Both starts are data, not faults."""
    c = Case(ilqg, name, 0, problem=problem)
    (s,) = c.history("mid")
    S = perturbed_starts(c.x0, 5, seed=37)
    clean = s.policy_rollout(S, trajectories=True)
    assert np.all(clean["ok"] == 1)
    P = S.copy()
    P[64, 2, 1] = np.nan
    P[5, 1, 0] = 1e200
    bad = s.policy_rollout(P, trajectories=True)
    assert bad["ok"][64, 2] == 0 and bad["ok"][5, 1] == 0
    keep = np.ones((B, 5), dtype=bool)
    keep[64, 2] = keep[5, 1] = False
    assert np.all(bad["ok"][keep] == 1)
    for k in clean:
        assert np.array_equal(bad[k][keep], clean[k][keep]), k
    costs = s.policy_rollout(P)
    assert np.array_equal(costs["ok"], bad["ok"]) and np.array_equal(costs["cost"][keep], clean["cost"][keep])
    c.close()


# ---------------------------------------------------------------------------
# 6. refusals
# ---------------------------------------------------------------------------
def test_refused_calls_name_the_argument_and_change_nothing(ilqg, torch):
    c = Case(ilqg, "carparking", 2, count=2)
    a, b = c.history("mid")
    S = perturbed_starts(c.x0, 3, seed=41)
    good = torch.from_numpy(S).cuda()
    cost = np.zeros((B, 3))
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream or None)

    def refused(call, *words):
        with pytest.raises(ilqg.IlqgError) as e:
            call()
        for w in words:
            assert w in str(e.value), (w, str(e.value))

    for n in (0, -1):
        refused(lambda: a._ck(a.lib.ilqg_batch_policy_rollout(a.h, n, C.c_void_p(S.ctypes.data), 1.0, 1, C.c_void_p(cost.ctypes.data), None, None, None, None)),
                "n_starts", "ilqg_batch_policy_rollout")
        refused(lambda: a._ck(a.lib.ilqg_batch_policy_rollout_device(a.h, n, C.c_void_p(good.data_ptr()), 1.0, 1, None, None, None, None, None, stream)),
                "n_starts", "ilqg_batch_policy_rollout_device")
    refused(lambda: a._ck(a.lib.ilqg_batch_policy_rollout(a.h, 3, None, 1.0, 1, C.c_void_p(cost.ctypes.data), None, None, None, None)), "x0")
    refused(lambda: a.policy_rollout(np.zeros((B, 0, c.nx))), "x0", "n_starts")
    refused(lambda: a.policy_rollout(np.zeros((B - 1, 3, c.nx))), "x0", "shape")
    refused(lambda: a.policy_rollout(np.zeros((B, 3, c.nx + 1))), "x0", "shape")
    refused(lambda: a.policy_rollout(torch.from_numpy(S), device=True), "x0", "host")
    refused(lambda: a.policy_rollout(S, device=True), "x0", "host")
    refused(lambda: a.policy_rollout(good), "x0", "device=True")
    refused(lambda: a.policy_rollout(good.float(), device=True), "x0", "float64")
    refused(lambda: a.policy_rollout(torch.zeros((B, 3, 2 * c.nx), dtype=torch.float64, device="cuda")[:, :, ::2], device=True), "x0", "contiguous")
    refused(lambda: a.policy_rollout(good[:-1].contiguous(), device=True), "x0", "shape")
    # all outputs NULL: nothing to do
    assert a.lib.ilqg_batch_policy_rollout(a.h, 3, C.c_void_p(S.ctypes.data), 1.0, 1, None, None, None, None, None) == 0
    assert a.lib.ilqg_batch_policy_rollout_device(a.h, 3, C.c_void_p(good.data_ptr()), 1.0, 1, None, None, None, None, None, stream) == 0
    a.iterate(2)
    b.iterate(2)
    assert_state_equal(state(a), state(b), "two iterations behind refused calls")
    c.close()
