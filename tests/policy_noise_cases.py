"""TEST INFRASTRUCTURE — the disturbance tables of policy_rollout(disturbance=...)'s tests and what its outputs are held
against: reference_disturbed_rollout, the reference's forward_pass (iLQG_func.tem:121-185) through the oracle driver ONE STEP AT
A TIME, with the disturbance behind each step,
    x_{k+1} <- x_next + w[k]        k = 0 .. N-1
built on the body of policy_cases.reference_rollout the way policy_cases.reference_plant is.  Leg k is a forward_pass over a horizon of ONE
step from the roll-out's current state about row k of the policy (x rows k and k + 1; the running multipliers of step k; of a
per-time-step parameter the values k and k + 1 — almix's vref window moved k on), and gives x[0] (the state the control was
applied at), u[0] (the clamped control), the step's cost and the next state x[1].  The final cost is that of the LAST leg: the
one horizon whose final cost the driver evaluates at the roll-out's end.  The reference evaluates it at the state it reached
itself, x[1] of that leg: with a last row w[N-1] != 0 the reference has no final cost at the disturbed end state, and
reference_disturbed_rollout refuses such a table.  The cases held to the reference have a zero last row.

Used by tests/test_policy_noise_recipe.py (no GPU: with a zero table the chain is one whole forward_pass bit for bit, and wrong
recipes miss the GPU test's bar by a wide margin) and tests/test_gpu_policy_noise.py.  Builds, B = 70, SLOTS, R = 5 and the
histories are those of tests/test_gpu_policy_rollout.py; the noise is plant_cases.noise, 0.01 N(0, I), seeded."""
import numpy as np

from oracle.harness import Driver
from plant_cases import noise
from policy_cases import reference_rollout

R = 5
SIGMA = 0.01
KINDS = [(0.0, 1), (1.0, 1), (0.0, 0)]  # (alpha, feedback) held to the reference


def tables(c, n_starts=R, seed=3, batch=None, last_zero=True, shared=False):
    """w [B, R, N, nx] (shared: [R, N, nx]): plant_cases.noise with sigma = 0.01; roll-out r = 0 of every trajectory gets a
    zero table, and with last_zero row N - 1 of every roll-out is zero (what is held to the reference)"""
    batch = (1 if shared else c.x0.shape[0]) if batch is None else batch
    w = noise(c, c.N, rounds=n_starts, batch=batch, seed=seed, sigma=SIGMA).reshape(batch, n_starts, c.N, c.nx)
    w[:, 0] = 0.0
    if last_zero:
        w[:, :, -1] = 0.0
    return np.ascontiguousarray(w[0] if shared else w)


def step_params(lib, n_hor):
    """the names of the problem's per-time-step parameters (size -1)"""
    d = Driver(lib, n_hor)
    try:
        return [name for name, size in d.param_desc() if size == -1]
    finally:
        d.close()


def reference_disturbed_rollout(lib, n_hor, params, opts, start, policy, alpha, feedback, w=None, cost=0.0, w_pen=(0.0, 0.0), multipliers=None,
                                moving=None):
    """(ok, cost, x [N+1, nx], u [N, nu], c [N+1]): forward_pass from `start` about `policy` = (x, u, l, L) under the
    disturbance table w [N, nx] (None: none), as the chain of N one-step legs the module's text describes.  cost is the sum of
    c from 0.0 in step order, the final cost last — forward_pass's own order.  ok = 0 as soon as a leg's forward_pass returns
    0; the later rows are then NaN.  moving: the per-time-step parameter names (step_params; looked up if None)."""
    x, u, l, L = (np.asarray(a, dtype=np.float64) for a in policy)
    N = n_hor
    if x.shape[0] == N:
        x = np.concatenate([x, x[-1:]])
    if w is not None:
        w = np.asarray(w, dtype=np.float64)
        assert w.shape == (N, x.shape[1])
        assert not np.any(w[-1]), "the reference has no final cost at a state it did not reach itself: the last row must be zero"
    moving = step_params(lib, 1) if moving is None else moving
    xs, us, cs = np.full((N + 1, x.shape[1]), np.nan), np.full((N, u.shape[1]), np.nan), np.full(N + 1, np.nan)
    state, total = np.asarray(start, dtype=np.float64).copy(), 0.0
    zl, zL = np.zeros_like(l[:1]), np.zeros_like(L[:1])
    # every leg is the body of policy_cases.reference_rollout at a horizon of one step, in ONE driver kept open for the chain
    # (a driver per leg costs ten times the leg; tests/test_policy_noise_recipe.py holds the two forms to equal bits)
    d = Driver(lib, 1, {n: v for n, v in params.items() if n not in moving}, opts)
    try:
        for k in range(N):
            for name in moving:
                d.set_param(name, np.asarray(params[name], dtype=np.float64)[k:k + 2])
            if d.init(state, u[k:k + 1]) != 1:
                return 0, float("nan"), xs, us, cs
            d.set_state(x[k:k + 2], u[k:k + 1], cost, 1.0, w_pen)
            if multipliers is not None:
                d.set_multipliers(np.asarray(multipliers[0])[k:k + 1], multipliers[1])
            if alpha == 0.0 and not feedback:
                ok, _ = d.forward_pass(0.0)
            else:
                d.set_gains(l[k:k + 1] if alpha != 0.0 else zl, L[k:k + 1] if feedback else zL)
                ok, _ = d.forward_pass(alpha if alpha != 0.0 else 1.0)
            if ok != 1:
                return 0, float("nan"), xs, us, cs
            (xr, ur), sc = d.traj(1), d.step_costs(1)
            xs[k], us[k], cs[k] = xr[0], ur[0], sc[0]
            total += sc[0]
            state = xr[1] if w is None else xr[1] + w[k]
    finally:
        d.close()
    xs[N], cs[N] = state, sc[1]
    total += sc[1]
    return 1, float(total), xs, us, cs


def leg_by_leg(lib, n_hor, params, opts, start, policy, alpha, feedback, w=None, cost=0.0, w_pen=(0.0, 0.0), multipliers=None, moving=()):
    """reference_disturbed_rollout with every leg a call of policy_cases.reference_rollout (a driver of its own per leg)"""
    x, u, l, L = (np.asarray(a, dtype=np.float64) for a in policy)
    N = n_hor
    xs, us, cs = np.full((N + 1, x.shape[1]), np.nan), np.full((N, u.shape[1]), np.nan), np.full(N + 1, np.nan)
    state, total = np.asarray(start, dtype=np.float64).copy(), 0.0
    for k in range(N):
        p = dict(params)
        for name in moving:
            p[name] = np.asarray(params[name], dtype=np.float64)[k:k + 2]
        mul = None if multipliers is None else (np.asarray(multipliers[0])[k:k + 1], multipliers[1])
        ok, _, xr, ur, sc = reference_rollout(lib, 1, p, opts, state, (x[k:k + 2], u[k:k + 1], l[k:k + 1], L[k:k + 1]), alpha, feedback,
                                              cost=cost, w_pen=w_pen, multipliers=mul, step_costs=True)
        assert ok == 1
        xs[k], us[k], cs[k] = xr[0], ur[0], sc[0]
        total += sc[0]
        state = xr[1] if w is None else xr[1] + np.asarray(w, dtype=np.float64)[k]
    xs[N], cs[N] = state, sc[1]
    total += sc[1]
    return 1, float(total), xs, us, cs


def worst(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.max(np.abs(a - b) / np.maximum(1.0, np.abs(b)))) if a.size else 0.0
