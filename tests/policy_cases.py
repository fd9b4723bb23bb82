"""TEST INFRASTRUCTURE — what BatchSolver.policy_rollout is compared against: the reference's own forward_pass
(iLQG_func.tem:121-185) through the oracle driver, started from another state than the planned one.

A policy is (x [N+1, nx], u [N, nu], l [N, nu], L [N, nu*nx]) with the cost, penalty weights and multipliers of its plan.
The four (alpha, feedback) combinations reach forward_pass through Driver.set_gains:
    feedback = 1, alpha != 0   forward_pass(alpha)
    feedback = 0, alpha  = 0   forward_pass(0)
    feedback = 1, alpha  = 0   l := 0, forward_pass(1)        u = u_nom + 0 * 1 + L dx
    feedback = 0, alpha != 0   L := 0, forward_pass(alpha)    u = u_nom + alpha l + 0 * dx
Used by tests/test_policy_rollout_recipe.py (which pins the recipe to the reference build) and
tests/test_gpu_policy_rollout.py."""
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


def reference_rollout(lib, n_hor, params, opts, start, policy, alpha, feedback, cost=0.0, w_pen=(0.0, 0.0), multipliers=None):
    """(ok, cost, x [N+1, nx], u [N, nu]) of forward_pass from `start` about `policy` = (x, u, l, L) in the driver build
    `lib`.  x may have N rows (a head): forward_pass reads the nominal states of the steps k < N only."""
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
    finally:
        d.close()
    return ok, c, xr, ur


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
