"""The control interval of a caller with its own plant: ilqg_batch_head / _head_device / _shift_device / _shift_param and
ilqg_multi_head ({iterate; read the heads; the plant's step; shift} without a field crossing to the host).

The feature moves data and runs kernels that existed before, so EVERY comparison is np.array_equal (bit for bit): a head
against the getters, the device forms against the host forms, the moved parameter window against set_param of the same
values.  Inputs, builds and history are those of tests/test_gpu_receding.py (B = 200: four tiles, a ragged last one;
init, then 7 iterations, which in CarParking's lane mapping leaves some current trajectories in kept roll-out planes of
the line search and others in X / U).  No test hands a host pointer to a _device entry.
"""
import ctypes as C
import os

import numpy as np
import pytest

import test_gpu_receding as base
from oracle.harness import CAR_PARAMS, almix_case

pytestmark = pytest.mark.gpu

BUILDS = [("carparking", 0), ("carparking", 2), ("carparking_wave", 0), ("hxtest", 0), ("synth16x8", 0), ("synth10hx", 0),
          ("almix", 0)]
B = 200
state, assert_state_equal = base.state, base.assert_state_equal


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


@pytest.fixture(scope="module")
def torch():
    import torch as t
    assert t.cuda.is_available()
    return t


class Case:
    """`count` solvers of one build with the same history: init, 7 iterations"""

    def __init__(self, ilqg, name, groups, count, batch=B):
        self.name = name
        problem, fd, strict, self.N, params, opts, self.x0, self.u0 = base.setup(name, batch)
        self.params = params
        kw = dict(batch=batch, n_hor=self.N, params=params, opts=dict(opts, max_iter=40), strict=strict, groups=groups)
        self.solvers = [ilqg.BatchSolver(problem, fd, **kw) for _ in range(count)]
        if groups:
            assert self.solvers[0].groups() == groups
        self.nx, self.nu = self.solvers[0].problem.nx, self.solvers[0].problem.nu

    def history(self):
        for s in self.solvers:
            s.init(self.x0, self.u0)
            s.iterate(7)
        if self.name == "carparking":
            # both locations occur (tests/test_gpu_receding.py): kept roll-out planes (ILQG_I_LOC != 0) and X / U — the
            # case a head read can get wrong
            acc, idx = self.solvers[0].ints("accepted"), self.solvers[0].ints("alpha_idx")
            assert np.any((acc == 1) & (idx <= 4)) and np.any((acc == 0) | (idx > 4))
        return self.solvers

    def close(self):
        for s in self.solvers:
            s.close()


def head_equal(a, b, what):
    assert sorted(a) == sorted(b), what
    for k in a:
        assert np.array_equal(np.asarray(a[k]), np.asarray(b[k])), "%s: %s differs" % (what, k)


def to_numpy(h):
    return {k: v.cpu().numpy() for k, v in h.items()}


# ---------------------------------------------------------------------------
# 1. the head equals the getters, and reading it changes nothing
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("name,groups", BUILDS)
def test_head_equals_the_getters(ilqg, name, groups):
    c = Case(ilqg, name, groups, 2)
    a, b = c.solvers
    for steps in (1, 5, c.N):
        c.history()
        h = a.head(steps, gains=True)  # first: the getters move every trajectory home
        l, L = a.gains()
        want = dict(x=a.x()[:, :steps], u=a.u()[:, :steps], l=l[:, :steps], L=L[:, :steps], cost=a.scalar("cost"))
        assert h["x"].shape == (B, steps, c.nx) and h["L"].shape == (B, steps, c.nu * c.nx) and h["cost"].shape == (B,)
        head_equal(h, want, "%s steps=%d" % (name, steps))
        h2 = a.head(steps)  # ... and with the trajectories at home, without the gains
        head_equal(h2, {k: want[k] for k in ("x", "u", "cost")}, "%s steps=%d, at home" % (name, steps))
        # no side effect: b had the same history and never called head
        c.history()
        a.head(steps, gains=True)
        a.iterate(3)
        b.iterate(3)
        assert_state_equal(state(a), state(b), "%s steps=%d: three iterations behind a head" % (name, steps))
    c.close()


# ---------------------------------------------------------------------------
# 2. the device head equals the host head
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("name,groups", BUILDS)
def test_device_head_equals_the_host_head(ilqg, torch, name, groups):
    c = Case(ilqg, name, groups, 1)
    (a,) = c.history()
    for steps in (1, 5):
        hd = a.head(steps, gains=True, device=True)
        assert all(v.is_cuda and v.dtype == torch.float64 for v in hd.values())
        hh = a.head(steps, gains=True)
        head_equal(to_numpy(hd), hh, "%s steps=%d" % (name, steps))
        # single outputs through the raw entry, every other pointer NULL
        stream = C.c_void_p(torch.cuda.current_stream().cuda_stream or None)
        x = torch.full((B, steps, c.nx), np.nan, dtype=torch.float64, device="cuda")
        cost = torch.full((B,), np.nan, dtype=torch.float64, device="cuda")
        assert a.lib.ilqg_batch_head_device(a.h, steps, C.c_void_p(x.data_ptr()), None, None, None, None, stream) == 0
        assert a.lib.ilqg_batch_head_device(a.h, steps, None, None, None, None, C.c_void_p(cost.data_ptr()), stream) == 0
        assert np.array_equal(x.cpu().numpy(), hh["x"]) and np.array_equal(cost.cpu().numpy(), hh["cost"])
    c.close()


# ---------------------------------------------------------------------------
# 3. the device shift equals the host shift
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("name,groups", BUILDS)
def test_device_shift_equals_the_host_shift(ilqg, torch, name, groups):
    c = Case(ilqg, name, groups, 2)
    dev, host = c.solvers
    rng = np.random.default_rng(6)
    cuda = lambda a: None if a is None else torch.from_numpy(a).cuda()
    for form in ("both", "x0", "neither"):
        for s in (1, 5, c.N - 1):
            c.history()
            x0_new = host.head(s + 1)["x"][:, s] + 0.01 * rng.standard_normal((B, c.nx)) if form != "neither" else None
            u_tail = 0.4 * rng.standard_normal((B, s, c.nu)) if form == "both" else None
            host.shift(s, x0_new, u_tail)
            if form == "neither":  # (no tensor for BatchSolver.shift to recognise: the device entry itself, both pointers NULL)
                assert dev.lib.ilqg_batch_shift_device(dev.h, s, None, None, C.c_void_p(torch.cuda.current_stream().cuda_stream or None)) == 0
            else:
                dev.shift(s, cuda(x0_new), cuda(u_tail))
            what = "%s %s s=%d" % (name, form, s)
            a = state(dev)
            assert_state_equal(a, state(host), what + " after the shift")
            if x0_new is not None:
                assert np.array_equal(a["x"][:, 0], x0_new)
            dev.iterate(5)
            host.iterate(5)
            assert_state_equal(state(dev), state(host), what + " five iterations on")
    # steps = 0 with x0 given
    c.history()
    x0_new = host.head(1)["x"][:, 0] + 0.01 * rng.standard_normal((B, c.nx))
    host.shift(0, x0_new)
    dev.shift(0, cuda(x0_new))
    assert_state_equal(state(dev), state(host), "%s steps = 0" % name)
    c.close()


# ---------------------------------------------------------------------------
# 4. stream order
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("name,groups", [("carparking", 2), ("synth16x8", 0)])
def test_device_entries_follow_the_callers_stream(ilqg, torch, name, groups):
    """The inputs are written, and the outputs read, by work that is only ENQUEUED on a side stream when the call is made.
    (This can catch a missing wait; it cannot fail a correct one.)"""
    c = Case(ilqg, name, groups, 2)
    dev, host = c.history()
    s = 5
    rng = np.random.default_rng(9)
    x0_final = host.head(s + 1)["x"][:, s] + 0.01 * rng.standard_normal((B, c.nx))
    x0_src = torch.from_numpy(x0_final).cuda()
    x0_t = torch.zeros((B, c.nx), dtype=torch.float64, device="cuda")
    m = torch.ones((4096, 4096), dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    s1 = torch.cuda.Stream()
    with torch.cuda.stream(s1):
        for _ in range(3):
            m = (m @ m) * 1e-4  # fp64 work ahead of the write: it is still pending when shift() returns
        x0_t.copy_(x0_src)
        dev.shift(s, x0_t)
    host.shift(s, x0_final)
    assert_state_equal(state(dev), state(host), "%s: x0 written on a side stream" % name)
    dev.iterate(2)
    host.iterate(2)
    with torch.cuda.stream(s1):
        for _ in range(3):
            m = (m @ m) * 1e-4
        h = {k: v.clone() for k, v in dev.head(s, gains=True, device=True).items()}
    s1.synchronize()
    head_equal(to_numpy(h), host.head(s, gains=True), "%s: head read on a side stream" % name)
    c.close()


# ---------------------------------------------------------------------------
# 5. the window of a per-time-step parameter
# ---------------------------------------------------------------------------
def almix_solvers(ilqg, count):
    c = Case(ilqg, "almix", 0, count)
    return c, np.asarray(c.params["vref"], dtype=np.float64)


def test_parameter_window_moves_with_the_horizon(ilqg):
    c, vref = almix_solvers(ilqg, 4)
    A, Bs, Cs, M = c.history()
    N, s = c.N, 4
    tail = 0.8 + 0.4 * np.sin(0.2 * (N + 1 + np.arange(s)))  # the formula of almix_case continued
    moved = np.concatenate([vref[s:], tail])
    A.shift_param("vref", s, tail)
    A.shift(s)
    Bs.set_param("vref", moved)
    Bs.shift(s)
    Cs.shift(s)
    # the host copy moved too: setting ANOTHER parameter (to the value it has) re-sends the whole table from it
    M.shift_param("vref", s, tail)
    M.set_param("h", c.params["h"])
    M.shift(s)
    for b in (A, Bs, Cs, M):
        b.iterate(5)
    a, b_, c_, m = state(A), state(Bs), state(Cs), state(M)
    assert_state_equal(a, b_, "shift_param against set_param of the moved window")
    assert_state_equal(m, b_, "shift_param, then set_param of another parameter")
    # vref enters through an equality constraint whose penalty is zero in the initial roll-out: compared after iterations.
    # (CPU oracle, this chain on every 25th of these starts: the cost is the same to the last bit behind the shift and
    # 0.2 to 2.4 apart, at a cost of about 5, five iterations on — 8 of 8 starts.)
    print("cost with the moved window / with the window left: largest difference %.3g" % np.max(np.abs(a["cost"] - c_["cost"])))
    assert not np.array_equal(a["cost"], c_["cost"])
    c.close()


def test_parameter_window_tail_rules(ilqg):
    c, vref = almix_solvers(ilqg, 2)
    A, Bs = c.solvers
    N = c.N
    tail_full = 0.5 + 0.01 * np.arange(N)
    for what, s, tail, moved in (("tail=None holds p[n_hor]", 7, None, np.concatenate([vref[7:], np.repeat(vref[-1:], 7)])),
                                 ("steps = 0", 0, None, vref),
                                 ("steps = n_hor", N, tail_full, np.concatenate([vref[N:], tail_full])),
                                 ("steps = n_hor, tail=None", N, None, np.repeat(vref[-1:], N + 1))):
        A.set_param("vref", vref)
        Bs.set_param("vref", vref)
        c.history()  # (pushes the table: the window then moves on the device)
        A.shift_param("vref", s, tail)
        Bs.set_param("vref", moved)
        A.shift(2)
        Bs.shift(2)
        A.iterate(5)
        Bs.iterate(5)
        assert_state_equal(state(A), state(Bs), what)
    c.close()


def test_parameter_window_before_the_first_push(ilqg):
    """a table that has not reached the device yet: the host copy moves, and that is what is sent"""
    params, opts, x0, u0 = almix_case(batch=8)
    vref, s = np.asarray(params["vref"]), 3
    kw = dict(batch=8, n_hor=u0.shape[1], params=params, opts=opts)
    a, b = ilqg.BatchSolver("almix", 1, **kw), ilqg.BatchSolver("almix", 1, **kw)
    a.shift_param("vref", s)
    b.set_param("vref", np.concatenate([vref[s:], np.repeat(vref[-1:], s)]))
    for q in (a, b):
        q.init(x0, u0)
        q.iterate(6)
    assert_state_equal(state(a), state(b), "moved before the first push")
    a.close()
    b.close()


# ---------------------------------------------------------------------------
# 6. errors
# ---------------------------------------------------------------------------
def test_refused_calls_name_the_argument_and_change_nothing(ilqg, torch):
    c, vref = almix_solvers(ilqg, 1)
    (a,) = c.history()
    N, nx, nu = c.N, c.nx, c.nu
    before = state(a)
    good_x0 = torch.zeros((B, nx), dtype=torch.float64, device="cuda")

    def refused(call, *words):
        with pytest.raises(ilqg.IlqgError) as e:
            call()
        for w in words:
            assert w in str(e.value), (w, str(e.value))

    for steps in (0, -1, N + 1):
        refused(lambda: a.head(steps), "steps", "n_hor")
        refused(lambda: a.head(steps, device=True), "steps", "n_hor")
    for steps in (-1, N, N + 1):
        refused(lambda: a.shift(steps, good_x0), "steps", "n_hor")
    for steps in (-1, N + 1):
        refused(lambda: a.shift_param("vref", steps), "steps", "n_hor")
    refused(lambda: a.shift_param("nosuch", 1), "nosuch", "is not a parameter of this problem")
    refused(lambda: a.shift_param("cu", 1), "cu", "time step")
    refused(lambda: a.shift_param("vref", 3, np.zeros(2)), "tail")
    refused(lambda: a.shift(1, good_x0.float()), "x0", "float64")
    refused(lambda: a.shift(1, torch.zeros((B, 2 * nx), dtype=torch.float64, device="cuda")[:, ::2]), "x0", "contiguous")
    refused(lambda: a.shift(1, torch.zeros((B - 1, nx), dtype=torch.float64, device="cuda")), "x0", "shape")
    refused(lambda: a.shift(2, good_x0, torch.zeros((B, 3, nu), dtype=torch.float64, device="cuda")), "u_tail", "shape")
    refused(lambda: a.shift(2, good_x0, torch.zeros((B, 2, nu), dtype=torch.float32, device="cuda")), "u_tail", "float64")
    refused(lambda: a.shift(2, good_x0, np.zeros((B, 2, nu))), "u_tail", "host")
    refused(lambda: a.shift(2, np.zeros((B, nx)), torch.zeros((B, 2, nu), dtype=torch.float64, device="cuda")), "x0", "host")
    assert_state_equal(state(a), before, "refused calls")
    # ... and the parameter window is where it was: one more iteration equals that of an untouched twin
    (b,) = Case(ilqg, "almix", 0, 1).history()
    a.iterate(1)
    b.iterate(1)
    assert_state_equal(state(a), state(b), "an iteration behind refused calls")
    b.close()
    c.close()


# ---------------------------------------------------------------------------
# 7. several shards
# ---------------------------------------------------------------------------
def test_multi_head_equals_the_single_batch(ilqg):
    from conftest import load_package
    N = 500
    x0, u0 = load_package().synth.car_batch(B, N, first=9)
    one = ilqg.BatchSolver("carparking", 0, batch=B, n_hor=N, params=CAR_PARAMS, opts=dict(max_iter=40))
    m = ilqg.MultiSolver("carparking", 0, batch=B, n_hor=N, devices=[0] * 3, params=CAR_PARAMS, opts=dict(max_iter=40))
    for b in (one, m):
        b.init(x0, u0)
        b.iterate(4)
    for steps in (1, 7):
        head_equal(m.head(steps, gains=True), one.head(steps, gains=True), "steps=%d" % steps)
        head_equal(m.head(steps), one.head(steps), "steps=%d, no gains" % steps)
    with pytest.raises(ilqg.IlqgError) as e:
        m.head(N + 1)
    assert "steps" in str(e.value) and "n_hor" in str(e.value)
    m.close()
    one.close()


# ---------------------------------------------------------------------------
# 8. the loop
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("name,groups", [("carparking", 0), ("synth16x8", 0)])
def test_loop_on_the_device_equals_the_loop_through_the_host(ilqg, torch, name, groups):
    """three control intervals {iterate(6); read the applied steps; plant; shift}: heads and the measured state stay on the
    GPU in one, cross the host as whole fields in the other.  The plant is x_meas = x[s] of the plan + fixed noise."""
    problem, fd, strict, N, params, opts, x0, u0 = base.setup(name, B)
    s = 10 if N == 500 else 5
    kw = dict(batch=B, n_hor=N, params=params, opts=dict(opts, max_iter=40), strict=strict, groups=groups)
    dev, hand = ilqg.BatchSolver(problem, fd, **kw), ilqg.BatchSolver(problem, fd, **kw)
    nx = dev.problem.nx
    noise = 0.01 * np.random.default_rng(12).standard_normal((3, B, nx))
    noise_t = torch.from_numpy(noise).cuda()
    dev.init(x0, u0)
    hand.init(x0, u0)
    for r in range(3):
        dev.iterate(6)
        h = dev.head(s + 1, device=True)
        x_meas = (h["x"][:, s] + noise_t[r]).contiguous()
        dev.shift(s, x_meas)
        hand.iterate(6)
        x, u, cost = hand.x(), hand.u(), hand.scalar("cost")
        hand.shift(s, x[:, s] + noise[r])
        assert np.array_equal(h["u"][:, :s].cpu().numpy(), u[:, :s]), "round %d: applied controls" % r
        assert np.array_equal(h["x"][:, :s].cpu().numpy(), x[:, :s]) and np.array_equal(h["cost"].cpu().numpy(), cost)
    assert_state_equal(state(dev), state(hand), "%s after the loop" % name)
    dev.close()
    hand.close()
