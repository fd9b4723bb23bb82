"""TEST INFRASTRUCTURE — what BatchSolver.policy_rollout is compared against: the reference's own forward_pass
(iLQG_func.tem:121-185) through the oracle driver, started from another state than the planned one.

A policy is (x [N+1, nx], u [N, nu], l [N, nu], L [N, nu*nx]) with the cost, penalty weights and multipliers of its plan.
The four (alpha, feedback) combinations reach forward_pass through Driver.set_gains:
    feedback = 1, alpha != 0   forward_pass(alpha)
    feedback = 0, alpha  = 0   forward_pass(0)
    feedback = 1, alpha  = 0   l := 0, forward_pass(1)        u = u_nom + 0 * 1 + L dx
    feedback = 0, alpha != 0   L := 0, forward_pass(alpha)    u = u_nom + alpha l + 0 * dx
Used by tests/test_policy_rollout_recipe.py (which pins the recipe to the reference build) and
tests/test_gpu_policy_rollout.py.

reference_plant is what BatchSolver.receding_plant's logs are compared against: the same forward_pass, one step at a time
from the plant's own state under the plant's parameters, with the disturbance behind each step
(tests/test_plant_reference_recipe.py pins it, tests/test_gpu_receding_plant.py and tests/test_gpu_params_batch.py use it)."""
import numpy as np

from oracle.harness import Driver

COMBOS = [(1.0, 1), (0.25, 1), (0.0, 0), (0.0, 1), (1.0, 0), (0.25, 0)]  # (alpha, feedback): the four kinds, alpha in {1, 0.25}
SIGMA = 0.1


def perturbed_starts(x0, R, seed, sigma=SIGMA):
    """[B, R, nx]: start 0 of every trajectory is its own x_0 bit for bit, the others x_0 + sigma N(0, I)"""
    x0 = np.asarray(x0, dtype=np.float64)
    rng = np.random.default_rng(seed)
    s = x0[:, None, :] + sigma * rng.standard_normal((x0.shape[0], R, x0.shape[1]))
    s[:, 0] = x0
    return np.ascontiguousarray(s)


def reference_rollout(lib, n_hor, params, opts, start, policy, alpha, feedback, cost=0.0, w_pen=(0.0, 0.0), multipliers=None, step_costs=False):
    """(ok, cost, x [N+1, nx], u [N, nu]) of forward_pass from `start` about `policy` = (x, u, l, L) in the driver build
    `lib`.  x may have N rows (a head): forward_pass reads the nominal states of the steps k < N only.  With step_costs
    also c [N+1]: the cost of every step as forward_pass left it, the final cost last (Driver.step_costs)."""
    x, u, l, L = (np.asarray(a, dtype=np.float64) for a in policy)
    if x.shape[0] == n_hor:
        x = np.concatenate([x, x[-1:]])
    d = Driver(lib, n_hor, params, opts)
    try:
        assert d.init(start, u) == 1, "the open-loop roll-out from this start is not finite"
        d.set_state(x, u, cost, 1.0, w_pen)
        if multipliers is not None:
            d.set_multipliers(*multipliers)
        if alpha == 0.0 and not feedback:
            ok, c = d.forward_pass(0.0)
        else:
            d.set_gains(l if alpha != 0.0 else np.zeros_like(l), L if feedback else np.zeros_like(L))
            ok, c = d.forward_pass(alpha if alpha != 0.0 else 1.0)
        xr, ur = d.traj(1)
        sc = d.step_costs(1) if step_costs else None
    finally:
        d.close()
    return (ok, c, xr, ur, sc) if step_costs else (ok, c, xr, ur)


def shifted(a, k):
    """rows k.. of a [n, ...] followed by k copies of its last row: what a plan's policy is k steps on"""
    a = np.asarray(a, dtype=np.float64)
    return a if k == 0 else np.concatenate([a[k:], np.repeat(a[-1:], k, axis=0)])


def reference_plant(lib, n_hor, params, opts, start, policy, feedback, steps, w=None, cost=0.0, w_pen=(0.0, 0.0), multipliers=None):
    """(x [steps, nx], u [steps, nu], c [steps], cost, x_end): the plant of one round of BatchSolver.receding_plant from
    `start` about `policy` = (x, u, l, L) under the PLANT's parameter dict `params`, as a chain of `steps` ONE-step
    roll-outs of the reference's forward_pass.  Step k starts from the plant's current state about the policy shifted by k
    rows (and padded with its last row; the running multipliers move with it), and gives x[0] (the state the control was
    applied at), u[0] (the clamped control), c[0] (the step's running cost) and the next state x[1] + w[k] (w [steps, nx] or
    None).  cost is the sum of c from 0.0 in step order — k_plant's order —, x_end the state behind the last step.
    The time index every step is evaluated at is 0: exact for a problem that reads it through per-time-step parameters
    only (the loop refuses those); tests/test_plant_reference_recipe.py holds the chain without w against the first
    `steps` steps of one forward_pass bit for bit, for every build it is used with."""
    x, u, l, L = (np.asarray(a, dtype=np.float64) for a in policy)
    xs, us, cs = [], [], []
    state, total = np.asarray(start, dtype=np.float64).copy(), 0.0
    for k in range(steps):
        mul = None if multipliers is None else (shifted(multipliers[0], k), multipliers[1])
        ok, _, xr, ur, sc = reference_rollout(lib, n_hor, params, opts, state, (shifted(x, k), shifted(u, k), shifted(l, k), shifted(L, k)), 0.0, feedback,
                                              cost=cost, w_pen=w_pen, multipliers=mul, step_costs=True)
        assert ok == 1, "step %d of the plant: the reference's roll-out from its state is not finite" % k
        xs.append(xr[0]), us.append(ur[0]), cs.append(sc[0])
        total += sc[0]
        state = xr[1] if w is None else xr[1] + np.asarray(w, dtype=np.float64)[k]
    return np.array(xs), np.array(us), np.array(cs), float(total), state


def first_control(policy, start, alpha, feedback):
    """u_0 before the clamp, as the formula states it: u_nom [+ alpha l] [+ L (x - x_nom), state by state]"""
    x, u, l, L = (np.asarray(a, dtype=np.float64) for a in policy)
    nu, nx = u.shape[1], x.shape[1]
    out = u[0].copy()
    if alpha != 0.0:
        out = u[0] + l[0] * alpha
    if feedback:
        for i in range(nx):
            dx = start[i] - x[0, i]
            for j in range(nu):
                out[j] += L[0, j + i * nu] * dx
    return out


def cpu_plan(lib, n_hor, params, opts, x0, u0, iterations):
    """a plan of the driver build `lib` and its policy: init and, with iterations = 0, calc_derivs + back_pass (gains about
    the plan itself), else a solve of that many iterations (behind an accepted step the gains are those about the previous
    nominal trajectory — as in the batch).  dict(policy, cost, w_pen, multipliers)"""
    d = Driver(lib, n_hor, params, dict(opts, max_iter=max(iterations, 1)))
    assert d.init(x0, u0) == 1
    if iterations == 0:
        assert d.calc_derivs() == 1
        d.back_pass()
    else:
        d.solve()
    x, u = d.traj(0)
    l, L = d.gains()
    out = dict(policy=(x, u, l, L), cost=d.scalars()["cost"], w_pen=(0.0, 0.0), multipliers=None)
    if hasattr(d.lib, "drv_get_multipliers"):
        el, fin, w = d.multipliers()
        out.update(w_pen=w, multipliers=(el, fin))
    d.close()
    return out
