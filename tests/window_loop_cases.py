"""TEST INFRASTRUCTURE — the cases of BatchSolver.receding(windows=...) / receding_plant(windows=...): the resident closed
loops in which the windows of the per-time-step parameters move with the horizon.  For tests/test_receding_windows_recipe.py
(no GPU: what the GPU tests compare against exists, is the reference's own roll-out and tells a moved window from an unmoved
one) and tests/test_gpu_receding_windows.py.

B = 70 (one full and one partly filled wavefront), compared slots 0, 63, 64, 69; rounds = 3, steps = 3, iterations = 3 unless a
test says otherwise; default_rng(59).  A TRACK is T [B, n_hor + 1 + rounds * steps], a reference per trajectory that goes on
beyond the horizon: the rows of set_param_steps_batch are T[:, :n_hor + 1], the futures of the loop T[:, n_hor + 1:], and the
window of round r, step k is T[:, r * steps + k : r * steps + k + n_hor + 1].
  almix, FULL_DDP 1, N = 80:  T[b][k] = (0.8 + 0.4 sin(0.2 k)) (1 + 0.05 N(0, 1)), the case's `vref` continued.
  brachi_hli, n = 64:         the case's `ymin` continued by nominal[-1] - 0.05 j, j = 1 .. rounds * steps, times the same
                              5 % factor element by element.
Every (b, k) is distinct, so a transposed, mis-strided or mis-offset future shows."""
import numpy as np

from param_steps_cases import BRACHI_N, STEP_NAME, B, SLOTS, setup  # noqa: F401
from policy_cases import reference_rollout, shifted

ROUNDS, STEPS, ITERATIONS = 3, 3, 3
SEED = 59
BAR = 1e-10  # the tree's single-pass bar: |d| <= BAR max(1, |ref|)
# (problem, FULL_DDP, FMA-free): the builds of the composition test; every one compares bit for bit (the same kernels plus copies)
BUILDS = [("almix", 1, False), ("almix", 1, True), ("brachi_hli", 0, False), ("brachi_hli", 1, False)]


def track(name, params, n_hor, rounds=ROUNDS, steps=STEPS, batch=B):
    """T [batch, n_hor + 1 + rounds * steps]"""
    more = rounds * steps
    if name == "almix":
        nominal = 0.8 + 0.4 * np.sin(0.2 * np.arange(n_hor + 1 + more))
        assert np.array_equal(nominal[:n_hor + 1], np.asarray(params["vref"], dtype=np.float64))
    elif name == "brachi_hli":
        window = np.asarray(params["ymin"], dtype=np.float64)
        nominal = np.concatenate([window, window[-1] - 0.05 * np.arange(1, more + 1)])
    else:
        raise ValueError(name)
    rng = np.random.default_rng(SEED)
    return np.ascontiguousarray(nominal[None, :] * (1.0 + 0.05 * rng.standard_normal((batch, nominal.size))))


def window(T, n_hor, at):
    """the windows [batch, n_hor + 1] that begin `at` values into the tracks"""
    return np.ascontiguousarray(T[..., at:at + n_hor + 1])


def dict_at(name, params, T, n_hor, b, at):
    """the parameter dict trajectory b plans (and its plant steps) under when its window begins `at` values into its track"""
    return dict(params, **{STEP_NAME[name]: window(T[b], n_hor, at)})


def close(got, want):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    return bool(np.all(np.abs(got - want) <= BAR * np.maximum(1.0, np.abs(want))))


def bars(got, want):
    """the smallest deviation, in bars, over the elements: how far a WRONG reference is from the right one at least"""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    return float(np.min(np.abs(got - want) / (BAR * np.maximum(1.0, np.abs(want)))))


def plant_chain(lib, name, n_hor, params, T, b, at, opts, start, policy, feedback, steps, w=None, cost=0.0, w_pen=(0.0, 0.0), multipliers=None,
                moving=True):
    """(x [steps, nx], u [steps, nu], c [steps], cost, x_end): policy_cases.reference_plant — a chain of ONE-step roll-outs of
    the reference's forward_pass, step k from the plant's current state about the policy and the running multipliers shifted
    by k rows — in which step k runs under trajectory b's window shifted by k as well (it begins at + k values into the
    track): the chain evaluates every step at time index 0, so the window has to move with the policy for step k to read
    p[name][k] of the round's window.  moving = False keeps the window where it is: every step reads p[name][0], the WRONG
    reference of tests/test_receding_windows_recipe.py."""
    x, u, l, L = (np.asarray(a, dtype=np.float64) for a in policy)
    xs, us, cs = [], [], []
    state, total = np.asarray(start, dtype=np.float64).copy(), 0.0
    for k in range(steps):
        mul = None if multipliers is None else (shifted(multipliers[0], k), multipliers[1])
        mine = dict_at(name, params, T, n_hor, b, at + (k if moving else 0))
        ok, _, xr, ur, sc = reference_rollout(lib, n_hor, mine, opts, state, (shifted(x, k), shifted(u, k), shifted(l, k), shifted(L, k)), 0.0, feedback,
                                              cost=cost, w_pen=w_pen, multipliers=mul, step_costs=True)
        assert ok == 1, "step %d of the plant: the reference's roll-out from its state is not finite" % k
        xs.append(xr[0]), us.append(ur[0]), cs.append(sc[0])
        total += sc[0]
        state = xr[1] if w is None else xr[1] + np.asarray(w, dtype=np.float64)[k]
    return np.array(xs), np.array(us), np.array(cs), float(total), state


def noise(nx, steps, rounds=ROUNDS, batch=B, sigma=0.01):
    """a disturbance behind every step, [batch, rounds * steps, nx]"""
    return sigma * np.random.default_rng(SEED + 1).standard_normal((batch, rounds * steps, nx))


def plant_starts(x0, sigma=0.1):
    """the plants' states at the start: x_0 + sigma N(0, I)"""
    x0 = np.asarray(x0, dtype=np.float64)
    return np.ascontiguousarray(x0 + sigma * np.random.default_rng(SEED + 2).standard_normal(x0.shape))


class WindowCase:
    """`count` solvers of one build on the case's inputs, every one with the rows T[:, :n_hor + 1] unless shared"""

    def __init__(self, ilqg, name, fd, strict=False, count=1, groups=0, batch=B, n=None, rounds=ROUNDS, steps=STEPS, opts=None):
        self.name, self.problem, self.fd, self.step = name, name, fd, STEP_NAME[name]
        self.N, self.params, self.opts, self.x0, self.u0 = setup(name, batch, n)
        self.rounds, self.steps = rounds, steps
        self.T = track(name, self.params, self.N, rounds, steps, batch)
        self.rows, self.future = window(self.T, self.N, 0), np.ascontiguousarray(self.T[:, self.N + 1:])
        kw = dict(batch=batch, n_hor=self.N, params=self.params, opts=dict(self.opts, max_iter=40, **(opts or {})), strict=strict, groups=groups)
        self.solvers = [ilqg.BatchSolver(name, fd, **kw) for _ in range(count)]
        if groups:
            assert self.solvers[0].groups() == groups

    def start(self, form="rows", b=0):
        """every solver initialised under the form's windows: "rows" (a window per trajectory) or "shared" (slot b's for all)"""
        for s in self.solvers:
            if form == "rows":
                s.set_param_steps_batch(self.step, self.rows)
            else:
                s.set_param(self.step, self.rows[b])
            s.init(self.x0, self.u0)
        return self.solvers

    def close(self):
        for s in self.solvers:
            s.close()
