"""BatchSolver.policy_rollout(noise=(seed, sigma)) and noise_table on the GPU: the roll-outs' process noise drawn on the device
from a seed (k_noise.inc; k_policy_drawn, k_noise_fill; ilqg_batch_policy_rollout_drawn, ilqg_batch_noise_table and their
device and multi forms).

The chain to the reference has two links.  (1) noise_table is held to the numpy restatement of the draw,
tests/noise_draw_cases.py (pinned without a GPU by tests/test_noise_draw_recipe.py), with the bar
    |d| <= 1e-12 sigma[i]   per entry:
the device's log, sincospi and sqrt are good to a few units in the last place, |ln ua| <= 22.9 and rho <= 6.76, so a normal is
off by about 1e-14 at most; the bar is 100 times that, and every mutant of the recipe misses it a million times.  Where
sigma[i] = 0 the entry is +0.0 or -0.0 exactly.  (2) The drawn roll-out is bit for bit policy_rollout(disturbance=
noise_table(...)) in cost, ok, x_end, x and u, and the table form is held to the reference's forward_pass by
tests/test_gpu_policy_noise.py.  The rest are identities, bit for bit: a draw depends on its counter alone.
Builds, B = 70, R = 5, SLOTS, the histories and the starts are those of tests/test_gpu_policy_rollout.py (its groups-and-shards
test's B = 200 for ours: four groups need more than three tiles); sigma is about 0.01 per component, the size of
tests/test_gpu_policy_noise.py's tables."""
import ctypes as C

import numpy as np
import pytest

import test_gpu_receding as base
from noise_draw_cases import table as recipe
from params_batch_cases import rows
from policy_cases import perturbed_starts
from policy_noise_cases import KINDS, R
from policy_param_cases import NAMED, SCALE, draws, limits_ordered
from test_gpu_policy_rollout import B, BUILDS, Case, ilqg, outputs_equal, to_numpy, torch  # noqa: F401

pytestmark = pytest.mark.gpu
state, assert_state_equal = base.state, base.assert_state_equal
KEYS = ("cost", "ok", "x_end", "x", "u")
SEED = (0x9E3779B9 << 32) | 0x7F4A7C15  # both halves of the key non-zero
TOP = 2 ** 32 - B                        # the last first_trajectory a batch of B admits
BAR = 1e-12
SLOTS = ("k_policy", "k_policy_params", "k_policy_drawn", "k_policy_drawn_params", "k_noise_fill")


def sigma_of(nx, zero=None):
    """about 0.01 per component, every component another value; `zero`: that component is not disturbed"""
    s = 0.01 * (1.0 + np.arange(nx) / nx)
    if zero is not None:
        s[zero] = 0.0
    return s


def launches(s):
    t = s.kernel_times()
    return {k: t[k][0] for k in SLOTS}


def both(s, S, W, noise, alpha=1.0, feedback=True, **kw):
    """(the drawn roll-out, the roll-out under the table W): the same call but for where the noise comes from"""
    drawn = s.policy_rollout(S, alpha, feedback, trajectories=True, noise=noise, **kw)
    kw = {k: v for k, v in kw.items() if k not in ("noise_shared", "first_trajectory")}
    return drawn, s.policy_rollout(S, alpha, feedback, trajectories=True, disturbance=W, **kw)


# ---------------------------------------------------------------------------
# 1. noise_table against the restatement
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["hxtest", "carparking", "synth10hx", "synth16x8"])  # N_X = 3, 4, 10, 16: a partial block, one, two and a half, four
def test_noise_table_is_the_recipe(ilqg, torch, name):
    c = Case(ilqg, name, 0)
    (s,) = c.solvers
    nx, N = c.nx, c.N
    assert nx == {"hxtest": 3, "carparking": 4, "synth10hx": 10, "synth16x8": 16}[name]
    sigma = sigma_of(nx, zero=1)
    sigma[0], sigma[-1] = 3.0, 1e-3
    live = sigma > 0
    seen = 0.0
    for seed, first, shared in ((0, 0, False), (SEED, 0, False), (SEED, TOP, False), (0, TOP, False), (SEED, 0, True), (SEED, TOP, True)):
        w = s.noise_table(R, seed, sigma, shared=shared, first_trajectory=first)
        want = recipe(B, R, N, nx, seed, sigma, shared=shared, first=first)
        assert w.shape == want.shape == ((R, N, nx) if shared else (B, R, N, nx))
        d = float(np.max(np.abs(w - want)[..., live] / sigma[live]))
        seen = max(seen, d)
        assert d <= BAR, "%s seed %#x first %d shared %d: worst |d| / sigma = %.3g" % (name, seed, first, shared, d)
        assert np.all(w[..., ~live] == 0.0) and np.all(np.isfinite(w))
        with torch.cuda.stream(torch.cuda.Stream()):
            t = s.noise_table(R, seed, sigma, shared=shared, first_trajectory=first, device=True).clone()
        torch.cuda.synchronize()
        assert np.array_equal(t.cpu().numpy(), w), "%s: device form against host form" % name
    full = s.noise_table(R, SEED, sigma)
    assert np.array_equal(s.noise_table(R, SEED, sigma, shared=True, first_trajectory=TOP), full[0])  # (shared: trajectory word 0, whatever first is)
    assert not np.array_equal(full[0], full[1]) and not np.array_equal(full, s.noise_table(R, SEED ^ (1 << 40), sigma))
    assert np.array_equal(s.noise_table(1, SEED, 0.5), s.noise_table(1, SEED, np.full(nx, 0.5)))  # (a scalar sigma: every component)
    print("%s (N_X = %d): worst |noise_table - recipe| / sigma = %.3g (bar %.0e)" % (name, nx, seen, BAR))
    c.close()


# ---------------------------------------------------------------------------
# 2. the drawn roll-out is the table roll-out
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("name,groups,strict", [(n, g, None) for n, g in BUILDS] + [("carparking", 0, True)])
def test_the_drawn_rollout_is_the_rollout_under_the_table(ilqg, torch, name, groups, strict):
    """every output, the three (alpha, feedback) kinds, per-trajectory and shared noise, the top of the trajectory word; costs
    only; with a parameter table of the roll-outs' own; the device form; nothing of the batch changes"""
    c = Case(ilqg, name, groups, count=2, strict=strict)
    s, twin = c.history("mid")
    S = perturbed_starts(c.x0, R, seed=23)
    sigma = sigma_of(c.nx)
    plain = s.policy_rollout(S, trajectories=True)
    for shared, first in ((False, 0), (True, 0), (False, TOP)):
        W = s.noise_table(R, SEED, sigma, shared=shared, first_trajectory=first)
        for alpha, feedback in (KINDS if not first else KINDS[:1]):
            drawn, table = both(s, S, W, (SEED, sigma), alpha, bool(feedback), noise_shared=shared, first_trajectory=first)
            outputs_equal(drawn, table, "%s shared=%d first=%d alpha=%g feedback=%d" % (name, shared, first, alpha, feedback), KEYS)
            assert drawn["ok"].any() and drawn["x"].shape == (B, R, c.N + 1, c.nx)
    assert not np.array_equal(drawn["x_end"], plain["x_end"]) and np.array_equal(drawn["x"][:, :, 0], S)
    W = s.noise_table(R, SEED, sigma)
    costs = s.policy_rollout(S, noise=(SEED, sigma))
    outputs_equal(costs, s.policy_rollout(S, disturbance=W), "%s: costs only" % name)
    assert sorted(costs) == ["cost", "ok", "x_end"]
    if name in NAMED:
        own = draws(c.params, NAMED[name], B, R, scale=SCALE[name])
        assert limits_ordered(own)
        drawn, table = both(s, S, W, (SEED, sigma), 0.25, True, params=own)
        outputs_equal(drawn, table, "%s: a parameter table of the roll-outs' own" % name, KEYS)
        assert not np.array_equal(drawn["cost"], costs["cost"])
    torch.cuda.synchronize()
    with torch.cuda.stream(torch.cuda.Stream()):
        x0_t = torch.from_numpy(S).to("cuda")
        d = {k: v.clone() for k, v in s.policy_rollout(x0_t, trajectories=True, device=True, noise=(SEED, sigma), noise_shared=True).items()}
    torch.cuda.synchronize()
    outputs_equal(to_numpy(d), s.policy_rollout(S, trajectories=True, noise=(SEED, sigma), noise_shared=True), "%s: device form against host form" % name)
    s.iterate(3)
    twin.iterate(3)
    assert_state_equal(state(s), state(twin), "%s: three iterations behind the drawn roll-outs" % name)
    c.close()


def test_the_drawn_rollout_under_per_trajectory_rows(ilqg):
    """under set_params_batch (the instantiations with the trajectory's row in front), without and with a table of the roll-outs' own"""
    c = Case(ilqg, "carparking", 0)
    (s,) = c.solvers
    _, mine = rows("carparking", c.params)
    s.set_params_batch(mine)
    c.history("mid")
    S = perturbed_starts(c.x0, R, seed=23)
    sigma = sigma_of(c.nx)
    W = s.noise_table(R, SEED, sigma, first_trajectory=7)
    drawn, table = both(s, S, W, (SEED, sigma), first_trajectory=7)
    outputs_equal(drawn, table, "per-trajectory rows", KEYS)
    own = draws(c.params, ("d", "cx"), B, R, seed=59, scale=SCALE["carparking"])
    drawn2, table2 = both(s, S, W, (SEED, sigma), params=own, first_trajectory=7)
    outputs_equal(drawn2, table2, "per-trajectory rows and a parameter table", KEYS)
    assert drawn["ok"].any() and not np.array_equal(drawn["cost"], drawn2["cost"])
    c.close()


# ---------------------------------------------------------------------------
# 3. bits depend on the counter alone
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["carparking", "synth16x8"])
def test_bits_do_not_depend_on_R_or_on_the_chunk(ilqg, name):
    c = Case(ilqg, name, 0)
    (s,) = c.history("mid")
    S = perturbed_starts(c.x0, 9, seed=23)
    sigma = sigma_of(c.nx)
    kw = dict(trajectories=True, noise=(SEED, sigma), first_trajectory=1000)
    nine, five = s.policy_rollout(S, **kw), s.policy_rollout(np.ascontiguousarray(S[:, :R]), **kw)
    outputs_equal(five, {k: nine[k][:, :R] for k in KEYS}, "%s: R = 5 against the first five of R = 9" % name, KEYS)
    assert np.array_equal(s.noise_table(9, SEED, sigma)[:, :R], s.noise_table(R, SEED, sigma))
    # slots 35 .. 69 as a batch of their own, drawn under first_trajectory + 35
    half = ilqg.BatchSolver(c.problem, c.fd, batch=B - 35, n_hor=c.N, params=c.params, opts=dict(c.opts, max_iter=40), strict=base.setup(name, B)[2])
    half.init(c.x0[35:], c.u0[35:])
    half.iterate(7)
    part = half.policy_rollout(np.ascontiguousarray(S[35:, :R]), trajectories=True, noise=(SEED, sigma), first_trajectory=1035)
    outputs_equal(part, {k: five[k][35:] for k in KEYS}, "%s: slots 35 .. 69 with first_trajectory + 35 against the whole batch" % name, KEYS)
    assert np.array_equal(half.noise_table(R, SEED, sigma, first_trajectory=35), s.noise_table(R, SEED, sigma)[35:])
    half.close()
    c.close()


def test_groups_and_shards_give_the_same_bits(ilqg):
    """1, 2 and 4 stream groups of one batch, and ilqg_multi_policy_rollout_drawn over three loop-back shards, with and without a
    parameter table; the table is the same whatever the groups"""
    n = 200
    cases = [Case(ilqg, "carparking", g, batch=n) for g in (0, 2, 4)]
    c = cases[0]
    S = perturbed_starts(c.x0, R, seed=29)
    sigma = sigma_of(c.nx)
    own = draws(c.params, NAMED["carparking"], n, R, scale=SCALE["carparking"])
    outs = []
    for q in cases:
        (s,) = q.history("mid")
        outs.append((s.policy_rollout(S, alpha=0.25, trajectories=True, noise=(SEED, sigma), first_trajectory=5),
                     s.policy_rollout(S, noise=(SEED, sigma), noise_shared=True),
                     s.policy_rollout(S, trajectories=True, noise=(SEED, sigma), params=own),
                     dict(w=s.noise_table(R, SEED, sigma, first_trajectory=5), ws=s.noise_table(R, SEED, sigma, shared=True))))
    for g, o in zip((2, 4), outs[1:]):
        for mine, first in zip(o, outs[0]):
            outputs_equal(mine, first, "groups = %d against groups = 0" % g)
    assert float(np.max(np.abs(outs[0][3]["w"] - recipe(n, R, c.N, c.nx, SEED, sigma, first=5)) / sigma)) <= BAR
    m = ilqg.MultiSolver("carparking", 0, batch=n, n_hor=c.N, devices=[0] * 3, params=c.params, opts=dict(max_iter=40))
    m.init(c.x0, c.u0)
    m.iterate(7)
    outputs_equal(m.policy_rollout(S, alpha=0.25, trajectories=True, noise=(SEED, sigma), first_trajectory=5), outs[0][0], "three shards against the single batch")
    outputs_equal(m.policy_rollout(S, noise=(SEED, sigma), noise_shared=True), outs[0][1], "three shards, shared noise")
    outputs_equal(m.policy_rollout(S, trajectories=True, noise=(SEED, sigma), params=own), outs[0][2], "three shards, a parameter table too")
    sg = (C.c_double * c.nx)(*sigma)
    with pytest.raises(ilqg.IlqgError) as e:  # the whole batch's range, before the first shard launches
        m._ck(m.lib.ilqg_multi_policy_rollout_drawn(m.h, R, S.ctypes.data_as(C.c_void_p), 0, None, None, 0, SEED, sg, 0, 2 ** 32 - n + 1, 1.0, 1,
                                                    np.zeros((n, R)).ctypes.data_as(C.c_void_p), None, None, None, None))
    assert "first_trajectory" in str(e.value)
    m.close()
    for q in cases:
        q.close()


# ---------------------------------------------------------------------------
# 4. launches and side effects
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("groups", [0, 2])
def test_a_drawn_call_launches_one_kernel_per_group_and_a_bad_start_fails_alone(ilqg, groups):
    c = Case(ilqg, "carparking", groups, count=2)
    a, twin = c.history("mid")
    S = perturbed_starts(c.x0, R, seed=37)
    sigma = sigma_of(c.nx)
    own = draws(c.params, ("d", "cx"), B, R, seed=59, scale=SCALE["carparking"])
    a.timing(True)
    n0 = launches(a)
    clean = a.policy_rollout(S, trajectories=True, noise=(SEED, sigma))
    n1 = launches(a)
    assert n1 == dict(n0, k_policy_drawn=n0["k_policy_drawn"] + a.groups()), (n0, n1)
    a.policy_rollout(S, noise=(SEED, sigma), params=own)
    n2 = launches(a)
    assert n2 == dict(n1, k_policy_drawn_params=n1["k_policy_drawn_params"] + a.groups()), (n1, n2)
    a.noise_table(R, SEED, sigma)
    a.noise_table(R, SEED, sigma, shared=True)  # (one table for all: written once, by the first group)
    assert launches(a) == dict(n2, k_noise_fill=n2["k_noise_fill"] + a.groups() + 1)
    a.timing(False)
    bad = S.copy()
    bad[64, 2, 0] = np.nan
    bad[5, 1, 3] = np.inf
    out = a.policy_rollout(bad, trajectories=True, noise=(SEED, sigma))
    keep = np.ones((B, R), dtype=bool)
    keep[64, 2] = keep[5, 1] = False
    assert out["ok"][64, 2] == 0 and out["ok"][5, 1] == 0 and np.array_equal(out["ok"][keep], clean["ok"][keep]) and clean["ok"][keep].all()
    for k in KEYS:
        assert np.array_equal(out[k][keep], clean[k][keep]), k
    a.iterate(2)
    twin.iterate(2)
    assert_state_equal(state(a), state(twin), "two iterations behind drawn roll-outs and tables")
    c.close()


def test_refused_calls_name_the_argument_and_launch_nothing(ilqg, torch):
    c = Case(ilqg, "almix", 0, count=2)
    a, b = c.history("mid")
    n, nx = 3, c.nx
    S = perturbed_starts(c.x0, n, seed=41)
    cost, W = np.zeros((B, n)), np.zeros((B, n, c.N, nx))
    good_x, good_w = torch.from_numpy(S).cuda(), torch.from_numpy(W).cuda()
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream or None)
    p = lambda v: v.ctypes.data_as(C.c_void_p)  # noqa: E731
    t = lambda v: C.c_void_p(v.data_ptr())  # noqa: E731
    sg = lambda *v: (C.c_double * nx)(*(v + (0.01,) * (nx - len(v))))  # noqa: E731
    names = lambda *s: (C.c_char_p * len(s))(*s)  # noqa: E731
    host, device = a.lib.ilqg_batch_policy_rollout_drawn, a.lib.ilqg_batch_policy_rollout_drawn_device
    table, table_device = a.lib.ilqg_batch_noise_table, a.lib.ilqg_batch_noise_table_device
    a.timing(True)
    n0 = launches(a)

    def refused(call, *words):
        with pytest.raises(ilqg.IlqgError) as e:
            a._ck(call())
        for w in words:
            assert w in str(e.value), (w, str(e.value))

    def rollout(x0=None, sigma=None, first=0, R_=n, form=host, names_=(0, None, None, 0), out=None, null_sigma=False, null_x0=False):
        x0 = (p(S) if form is host else t(good_x)) if x0 is None else x0
        out = (p(cost) if form is host else None) if out is None else out
        tail = (stream,) if form is device else ()
        return lambda: form(a.h, R_, None if null_x0 else x0, *names_, SEED, None if null_sigma else (sigma or sg()), 0, first, 1.0, 1, out, None, None, None,
                            None, *tail)

    for form, who in ((host, "ilqg_batch_policy_rollout_drawn"), (device, "ilqg_batch_policy_rollout_drawn_device")):
        refused(rollout(form=form, null_sigma=True), "sigma", who)
        refused(rollout(form=form, sigma=sg(0.5, -1.0)), "sigma[1]", "negative")
        refused(rollout(form=form, sigma=sg(float("nan"))), "sigma[0]", "finite")
        refused(rollout(form=form, sigma=sg(0.5, 0.5, float("inf"))), "sigma[2]", "finite")
        refused(rollout(form=form, first=-1), "first_trajectory", "negative")
        refused(rollout(form=form, first=2 ** 32 - B + 1), "first_trajectory", "2^32")
        for bad in (0, -1):
            refused(rollout(form=form, R_=bad), "n_starts", who)
        refused(rollout(form=form, null_x0=True), "x0")
    refused(rollout(names_=(1, names(b"nosuch"), p(np.ones((B, n, 2))), 0)), "names[0]", "nosuch", "_drawn")
    refused(rollout(names_=(1, names(b"vref"), p(np.ones((B, n, 2))), 0)), "names[0]", "vref", "time step")
    # host memory given to the device forms
    refused(rollout(form=device, x0=p(S)), "x0", "device memory")
    refused(rollout(form=device, out=p(cost)), "cost", "device memory")
    refused(lambda: table_device(a.h, n, SEED, sg(), 0, 0, p(W), stream), "w", "device memory")
    for form, tail, w in ((table, (), p(W)), (table_device, (stream,), t(good_w))):
        refused(lambda: form(a.h, n, SEED, None, 0, 0, w, *tail), "sigma", "ilqg_batch_noise_table")
        refused(lambda: form(a.h, n, SEED, sg(-0.0, -1e-300), 0, 0, w, *tail), "sigma[1]", "negative")
        refused(lambda: form(a.h, n, SEED, sg(), 0, -5, w, *tail), "first_trajectory")
        refused(lambda: form(a.h, n, SEED, sg(), 0, 2 ** 32 - B + 1, w, *tail), "first_trajectory", "2^32")
        refused(lambda: form(a.h, 0, SEED, sg(), 0, 0, w, *tail), "n_starts")
        refused(lambda: form(a.h, n, SEED, sg(), 0, 0, None, *tail), "w")
    for call, words in ((lambda: a.policy_rollout(S, noise=(SEED, sg()[:]), disturbance=W), ("noise", "disturbance")),
                        (lambda: a.policy_rollout(S, noise=(SEED, [0.01] * (nx + 1))), ("sigma", "shape")),
                        (lambda: a.policy_rollout(good_x, device=True, noise=(SEED, -0.5)), ("sigma", "negative")),
                        (lambda: a.noise_table(n, SEED, 0.01, first_trajectory=2 ** 32), ("first_trajectory",))):
        with pytest.raises(ilqg.IlqgError) as e:
            call()
        assert all(w in str(e.value) for w in words), str(e.value)
    # all outputs NULL: nothing to do, after the checks
    assert host(a.h, n, p(S), 0, None, None, 0, SEED, sg(), 0, 0, 1.0, 1, None, None, None, None, None) == 0
    assert launches(a) == n0, "a refused call launched a kernel"
    assert rollout(first=2 ** 32 - B)() == 0 and launches(a) == dict(n0, k_policy_drawn=n0["k_policy_drawn"] + a.groups())
    a.timing(False)
    a.iterate(2)
    b.iterate(2)
    assert_state_equal(state(a), state(b), "two iterations behind refused calls")
    c.close()
