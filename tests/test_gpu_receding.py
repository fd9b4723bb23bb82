"""Receding horizon on the device: ilqg_batch_shift / ilqg_batch_receding / ilqg_multi_shift.

A shift followed by a re-plan is what a caller of the reference's MEX entry does between two calls (u_nom = [u(:, s+1:end),
tail] and the new x0, iLQG_mex.c:113-120), so every result is defined by a composition of calls that existed before:
get_x / get_u, a numpy shift, set_x0 / set_u, init.  The device path must equal that composition BIT FOR BIT (it moves
data and then runs the same initial roll-out); against the reference's fixtures (tests/golden/receding_*.npz) the bars are
those of tests/test_gpu_parity.py: single passes 1e-10 * max(1, |ref|), a full solve's final cost rel 1e-6.
"""
import os

import numpy as np
import pytest

from conftest import golden
from oracle.harness import CAR_PARAMS, HX_N, HX_PARAMS, SYN10_PARAMS, SYN_PARAMS_TIGHT, almix_case, hx_inputs, syn10_inputs, syn_inputs
from receding_cases import CASES, case

pytestmark = pytest.mark.gpu

TOL = 1e-10  # single passes (tests/test_gpu_parity.py)


def close(a, b, tol=TOL):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return bool(np.all(np.abs(a - b) <= tol * np.maximum(1.0, np.abs(b))))


def worst(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.max(np.abs(a - b) / np.maximum(1.0, np.abs(b))))


@pytest.fixture(scope="module")
def ilqg():
    import __graft_entry__ as g
    g.load_package()
    from ddp_generator_amd import ilqg as m
    if not all(os.path.exists(m.library_path(p, fd, st)) for p, fd, st in
               (("carparking", 0, False), ("carparking", 0, "wave"), ("hxtest", 1, False), ("synth16x8", 1, False),
                ("synth10hx", 0, False), ("almix", 1, False))):
        g.build()
    if m.Problem("carparking", 0).device_count() < 1:
        pytest.fail("no HIP device visible: the GPU tests must run on the MI355X box")
    return m


def setup(name, batch, n_hor=None):
    """(problem, fd, strict, n_hor, params, opts, x0, u0) of a batch of `batch` starts; n_hor: the problem's usual horizon"""
    if name in ("carparking", "carparking_wave"):
        from conftest import load_package
        N = n_hor or 500
        x0, u0 = load_package().synth.car_batch(batch, N, first=40)
        # the second half starts four times as far out with ten times the control noise: by the seventh iteration a few of these
        # accept a step size of the line search's SECOND stage (CPU oracle: 4 of 100), the others one of the first
        x0[batch // 2:] *= 4.0
        u0[batch // 2:] *= 10.0
        return "carparking", 0, ("wave" if name == "carparking_wave" else False), N, CAR_PARAMS, {}, x0, u0
    if name == "hxtest":
        x0, u0 = hx_inputs(batch)
        return "hxtest", 1, False, HX_N, HX_PARAMS, {}, x0, u0
    if name == "synth16x8":
        N = n_hor or 60
        x0, u0 = syn_inputs(batch, N)
        return "synth16x8", 1, False, N, SYN_PARAMS_TIGHT, {}, x0, u0
    if name == "synth10hx":
        x0, u0 = syn10_inputs(batch, 50)
        return "synth10hx", 0, False, 50, SYN10_PARAMS, {}, x0, u0
    if name == "almix":
        params, opts, x0, u0 = almix_case(batch=batch)
        return "almix", 1, False, u0.shape[1], params, opts, x0, u0
    raise ValueError(name)


def state(s):
    """everything the issue's bit-for-bit comparison names"""
    out = dict(x=s.x(), u=s.u(), cost=s.scalar("cost"), lam=s.scalar("lambda"), status=s.ints("status"),
               iterations=s.ints("iterations"))
    if sum(s.multiplier_dims()) > 0:
        out["mul_running"], out["mul_final"] = s.multipliers()
        out["w_pen_l"], out["w_pen_f"] = s.scalar("w_pen_l"), s.scalar("w_pen_f")
    return out


def assert_state_equal(a, b, what):
    for k in a:
        assert np.array_equal(a[k], b[k]), "%s: %s differs" % (what, k)


# ---------------------------------------------------------------------------
# 1. the device shift equals the composition through the host, bit for bit
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("name,groups", [("carparking", 0), ("carparking", 2), ("carparking_wave", 0), ("hxtest", 0),
                                         ("synth16x8", 0), ("synth10hx", 0), ("almix", 0)])
def test_shift_equals_the_host_composition(ilqg, name, groups):
    """Two batches with the same history (init, 7 iterations: in the lane mapping the current trajectories of the steps
    accepted in the first stage of the line search then live in kept roll-out planes, ILQG_I_LOC != 0, the others in X / U).  One is shifted on the device; the other through the host:
    get_x / get_u (which first move every trajectory home), numpy, set_x0 / set_u, init.  Every argument form (x0 and tail
    given, x0 only, neither) with steps in {1, 5, N - 1}; B = 200 is not a multiple of 64."""
    B = 200
    problem, fd, strict, N, params, opts, x0, u0 = setup(name, B)
    rng = np.random.default_rng(5)
    kw = dict(batch=B, n_hor=N, params=params, opts=dict(opts, max_iter=40), strict=strict, groups=groups)
    dev, host = ilqg.BatchSolver(problem, fd, **kw), ilqg.BatchSolver(problem, fd, **kw)
    if groups:
        assert dev.groups() == groups
    nx, nu = dev.problem.nx, dev.problem.nu
    for form in ("both", "x0", "neither"):
        for s in (1, 5, N - 1):
            for b in (dev, host):
                b.init(x0, u0)
                b.iterate(7)
            acc, idx = dev.ints("accepted"), dev.ints("alpha_idx")
            print("%s %s s=%d: %d of %d steps accepted in the last iteration, %d active" % (name, form, s, int(acc.sum()), B, dev.active()))
            if name == "carparking":
                # both locations occur: a step accepted in the first stage leaves the trajectory in a kept roll-out plane
                # (ILQG_I_LOC != 0); one accepted in the second stage, or rejected, leaves it in X / U.  (No CarParking
                # start tried rejects a step this early; the second stage's acceptances give the mix.)
                assert np.any((acc == 1) & (idx <= 4)) and np.any((acc == 0) | (idx > 4))
            xh, uh = host.x(), host.u()
            x0_new = xh[:, s] + 0.01 * rng.standard_normal((B, nx)) if form != "neither" else None
            u_tail = 0.4 * rng.standard_normal((B, s, nu)) if form == "both" else None
            dev.shift(s, x0_new, u_tail)
            tail = u_tail if u_tail is not None else np.repeat(uh[:, -1:], s, axis=1)
            host.init(x0_new if x0_new is not None else xh[:, s], np.concatenate([uh[:, s:], tail], axis=1))
            a, b = state(dev), state(host)
            assert_state_equal(a, b, "%s %s s=%d after the shift" % (name, form, s))
            assert np.all(a["iterations"] == 0) and np.all((a["status"] == 0) | (a["status"] == 7))
            assert np.array_equal(a["x"][:, 0], x0_new if x0_new is not None else xh[:, s])
            dev.iterate(5)
            host.iterate(5)
            assert_state_equal(state(dev), state(host), "%s %s s=%d five iterations on" % (name, form, s))
    # steps = 0 with neither pointer is init
    for b in (dev, host):
        b.init(x0, u0)
        b.iterate(3)
    xh, uh = host.x(), host.u()
    dev.shift(0)
    host.init(xh[:, 0], uh)
    assert_state_equal(state(dev), state(host), "steps = 0")
    dev.close()
    host.close()


@pytest.mark.parametrize("name,N", [("carparking", 6), ("carparking", 64), ("carparking", 65), ("carparking", 130),
                                    ("carparking_wave", 6), ("carparking_wave", 64), ("carparking_wave", 65), ("carparking_wave", 130),
                                    ("synth16x8", 31), ("synth16x8", 32), ("synth16x8", 33)])
def test_shift_at_the_kernels_boundaries(ilqg, name, N):
    """The plain shift where its kernels' loops end (the shapes of test_gpu_best_of's boundary test, whose kernels share
    these loops): n_hor = 6, 64, 65, 130 is one, exactly one, one plus one and three rounds of k_shift_lane's 64 steps, and
    one to three blocks of k_shift_wave's 256 / N_U = 128 steps; synth16x8 (N_U = 8) at 31, 32, 33 lies around that form's
    block of 32 steps.  B = 72: a tail tile of 8 lanes.  steps in {1, n_hor - 1}, x0 and tail given or neither; against the
    composition through the host, bit for bit, right after the shift and two iterations on.
    Where the plans lie: after the three iterations in front of the first shift every plan of these starts lies in a kept
    roll-out plane in the lane mapping (printed; measured up to twelve iterations: 72 of 72 at n_hor = 6, 64 and 65, 71 of 72
    at 130 from the eleventh on), which k_shift_lane only copies.  So each case shifts a SECOND time at once: the first shift
    has brought every plan home to X / U, and the second moves all of them IN PLACE, which is what the rounds' order and
    barrier are for."""
    B = 72
    problem, fd, strict, N, params, opts, x0, u0 = setup(name, B, N)
    rng = np.random.default_rng(N)
    kw = dict(batch=B, n_hor=N, params=params, opts=dict(opts, max_iter=40), strict=strict)
    dev, host = ilqg.BatchSolver(problem, fd, **kw), ilqg.BatchSolver(problem, fd, **kw)
    nx, nu = dev.problem.nx, dev.problem.nu
    for s in (1, N - 1):
        for form in ("both", "neither"):
            for b in (dev, host):
                b.init(x0, u0)
                b.iterate(3)
            acc, idx = dev.ints("accepted"), dev.ints("alpha_idx")
            plane = (acc == 1) & (idx <= 4)  # (test_shift_equals_the_host_composition: where the current trajectory lives)
            print("%s N=%d s=%d %s: %d of %d trajectories in a kept roll-out plane" % (name, N, s, form, int(plane.sum()), B))
            for turn in ("from where the iterations left the plans", "again, in place"):
                xh, uh = host.x(), host.u()
                x0_new = xh[:, s] + 0.01 * rng.standard_normal((B, nx)) if form == "both" else None
                u_tail = 0.4 * rng.standard_normal((B, s, nu)) if form == "both" else None
                dev.shift(s, x0_new, u_tail)
                tail = u_tail if u_tail is not None else np.repeat(uh[:, -1:], s, axis=1)
                host.init(x0_new if x0_new is not None else xh[:, s], np.concatenate([uh[:, s:], tail], axis=1))
                what = "%s N=%d s=%d %s" % (name, N, s, form)
                assert_state_equal(state(dev), state(host), what + " after the shift " + turn)
            dev.iterate(2)
            host.iterate(2)
            assert_state_equal(state(dev), state(host), what + " two iterations on")
    dev.close()
    host.close()


# ---------------------------------------------------------------------------
# 2. against the reference's fixtures
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", CASES)
def test_shift_and_warm_solve_against_the_reference(ilqg, name):
    """The reference's solved plan goes in with set_x / set_u; shift(s) must give the reference's x0', clamped shifted u,
    rolled-out x and cost (single-pass bar).  The warm solve that follows exits as the reference's does, and where it took
    the reference's number of iterations its final cost agrees within rel 1e-6 (at least one of the three must)."""
    g, c = golden("receding_%s.npz" % name), case(name)
    s = ilqg.BatchSolver(c["problem"], c["fd"], batch=3, n_hor=c["n"], params=c["params"], opts=c["opts"])
    s.set_x(g["plan_x"])
    s.set_u(g["plan_u"])
    s.shift(int(g["s"]))
    x, u, cost = s.x(), s.u(), s.scalar("cost")
    print("%s: worst deviation x0' %.3g, u %.3g, x %.3g, cost %.3g" % (name, worst(x[:, 0], g["shift_x0"]), worst(u, g["init_u"]),
                                                                   worst(x, g["init_x"]), worst(cost, g["init_cost"])))
    assert np.array_equal(x[:, 0], g["shift_x0"])
    assert close(u, g["init_u"]) and close(x, g["init_x"]) and close(cost, g["init_cost"])
    assert np.all(s.ints("status") == 0) and np.all(s.ints("iterations") == 0)
    s.solve()
    iters, cost, rc = s.ints("iterations"), s.scalar("cost"), s.success()
    rel = np.abs(cost - g["warm_cost"]) / np.abs(g["warm_cost"])
    print("%s: iterations %s (reference %s), return values %s (reference %s), final cost rel. deviation %s" % (
        name, iters.tolist(), g["warm_iters"].astype(int).tolist(), rc.tolist(), g["warm_rc"].tolist(), rel.tolist()))
    assert np.array_equal(rc, g["warm_rc"])
    same = iters == g["warm_iters"].astype(int)
    assert same.any()
    assert np.all(rel[same] < 1e-6)
    s.close()


# ---------------------------------------------------------------------------
# 3. warm starts help
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("name,batch", [("carparking", 12), ("hxtest", 8), ("synth16x8", 6)])
def test_warm_start_needs_fewer_iterations(ilqg, name, batch):
    """solve cold, shift, solve warm: median warm iterations <= 0.75 x median cold (the reference build gives 0.52, 0 and
    0.48 on exactly these inputs; medians, because single free-running solves diverge between builds)"""
    c = case(name, batch)
    s = ilqg.BatchSolver(c["problem"], c["fd"], batch=batch, n_hor=c["n"], params=c["params"], opts=c["opts"])
    s.init(c["x0"], c["u0"])
    s.solve()
    cold = s.ints("iterations").copy()
    s.shift(c["s"])
    s.solve()
    warm = s.ints("iterations")
    print("%s: iterations cold %s, warm %s; medians %.1f / %.1f" % (name, cold.tolist(), warm.tolist(), np.median(cold), np.median(warm)))
    assert np.median(warm) <= 0.75 * np.median(cold)
    s.close()


# ---------------------------------------------------------------------------
# 4. the loop on the device
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("name,groups", [("carparking", 0), ("carparking", 2), ("carparking_wave", 0), ("synth16x8", 0)])
def test_receding_equals_the_hand_written_loop(ilqg, name, groups):
    B, rounds, iterations = 200, 3, 6
    problem, fd, strict, N, params, opts, x0, u0 = setup(name, B)
    s = 10 if N == 500 else 5
    kw = dict(batch=B, n_hor=N, params=params, opts=dict(opts, max_iter=40), strict=strict, groups=groups)
    dev, hand = ilqg.BatchSolver(problem, fd, **kw), ilqg.BatchSolver(problem, fd, **kw)
    dev.init(x0, u0)
    hand.init(x0, u0)
    out = dev.receding(rounds, s, iterations)
    xs, us, costs, starts = [], [], [], []
    for r in range(rounds):
        starts.append(hand.x()[:, 0])
        hand.iterate(iterations)
        xs.append(hand.x()[:, :s]), us.append(hand.u()[:, :s]), costs.append(hand.scalar("cost"))
        hand.shift(s)
    assert np.array_equal(out["x"], np.concatenate(xs, axis=1)) and np.array_equal(out["u"], np.concatenate(us, axis=1))
    assert np.array_equal(out["cost"], np.stack(costs, axis=1))
    for r in range(rounds):
        assert np.array_equal(out["x"][:, r * s], starts[r])
    assert np.array_equal(starts[0], x0)
    assert_state_equal(state(dev), state(hand), "after the loop")
    dev.close()
    hand.close()


def test_receding_refuses_per_step_parameters(ilqg):
    params, opts, x0, u0 = almix_case(batch=4)
    s = ilqg.BatchSolver("almix", 1, batch=4, n_hor=u0.shape[1], params=params, opts=opts)
    s.init(x0, u0)
    with pytest.raises(ilqg.IlqgError) as e:
        s.receding(2, 4, 3)
    assert "ilqg_batch_shift" in str(e.value) and "ilqg_batch_set_param" in str(e.value) and "vref" in str(e.value)
    s.close()


# ---------------------------------------------------------------------------
# 5. errors, several shards
# ---------------------------------------------------------------------------
def test_shift_refuses_bad_step_counts(ilqg):
    from conftest import load_package
    x0, u0 = load_package().synth.car_batch(4, 500)
    s = ilqg.BatchSolver("carparking", 0, batch=4, n_hor=500, params=CAR_PARAMS)
    s.init(x0, u0)
    before = state(s)
    for steps in (-1, 500, 501):
        with pytest.raises(ilqg.IlqgError) as e:
            s.shift(steps)
        assert "steps" in str(e.value) and "n_hor" in str(e.value)
        with pytest.raises(ilqg.IlqgError):
            s.receding(2, steps, 1)
    with pytest.raises(ilqg.IlqgError):
        s.receding(2, 0, 1)
    assert_state_equal(state(s), before, "a refused call")
    s.close()


def test_multi_shift_equals_the_single_batch(ilqg):
    """ilqg_multi_shift on three shards of one device (a ragged last one), every argument form"""
    from conftest import load_package
    B, N, s = 200, 500, 7
    x0, u0 = load_package().synth.car_batch(B, N, first=9)
    rng = np.random.default_rng(8)
    one = ilqg.BatchSolver("carparking", 0, batch=B, n_hor=N, params=CAR_PARAMS, opts=dict(max_iter=40))
    m = ilqg.MultiSolver("carparking", 0, batch=B, n_hor=N, devices=[0] * 3, params=CAR_PARAMS, opts=dict(max_iter=40))
    for form in ("both", "x0", "neither"):
        for b in (one, m):
            b.init(x0, u0)
            b.iterate(4)
        x0_new = rng.standard_normal((B, 4)) if form != "neither" else None
        u_tail = 0.4 * rng.standard_normal((B, s, 2)) if form == "both" else None
        one.shift(s, x0_new, u_tail)
        m.shift(s, x0_new, u_tail)
        assert np.array_equal(m.x(), one.x()) and np.array_equal(m.u(), one.u()) and np.array_equal(m.costs(), one.scalar("cost"))
        assert np.array_equal(m.ints("iterations"), one.ints("iterations")) and np.array_equal(m.ints("status"), one.ints("status"))
        one.iterate(3)
        m.iterate(3)
        assert np.array_equal(m.x(), one.x()) and np.array_equal(m.costs(), one.scalar("cost"))
    with pytest.raises(ilqg.IlqgError):
        m.shift(N)
    m.close()
    one.close()
