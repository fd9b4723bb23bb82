"""TEST INFRASTRUCTURE — the cases of BatchSolver.set_params_batch, for tests/test_params_batch_recipe.py (no GPU: what the GPU
tests compare against exists and is no no-op) and tests/test_gpu_params_batch.py.

Builds: the lane-mapped ones — CarParking with FULL_DDP 0 and 1, hxtest (limits that depend on the state), almix (multipliers;
its `vref` has a value per time step and stays shared), and the FMA-free CarParking.  Batch, slots, inputs and histories are
those of tests/test_gpu_policy_rollout.py (B = 70: one full and one partly filled wavefront; SLOTS = 0, 63, 64, 69); the draws
are the 5 % draws of tests/policy_param_cases.py with row [:, 1] as trajectory b's row (row [:, 0] is the nominal values)."""
import numpy as np

import test_gpu_receding as base
from policy_param_cases import NAMED, SCALE, draws, limits_ordered, params_of
from test_gpu_policy_rollout import B, SLOTS, Case

# (name of base.setup, FULL_DDP, strict)
BUILDS = [("carparking", 0, False), ("carparking", 1, False), ("hxtest", 1, False), ("almix", 1, False), ("carparking", 0, True)]
CPU_BUILDS = BUILDS[:4]  # (the FMA-free build is the same problem on the CPU)
ALPHAS = (1.0, 0.3727594, 0.1389495, 0.0517947, 0.0193070, 0.0071969, 0.0026827, 0.0010000)  # standard_parameters() (iLQG.c:57-78)


def setup(name, fd, batch=B):
    """(problem, n_hor, params, opts, x0, u0): tests/test_gpu_receding.py's inputs, for either FULL_DDP of CarParking"""
    problem, fd0, strict, N, params, opts, x0, u0 = base.setup(name, batch)
    assert fd == fd0 or name == "carparking"
    return problem, N, params, opts, x0, u0


def rows(name, params, batch=B, seed=None, names=None):
    """(table {name: [batch, 2, size]}, rows {name: [batch, size]}): trajectory b's row is row 1 of its draw"""
    kw = {} if seed is None else dict(seed=seed)
    t = draws(params, names or NAMED[name], batch, 2, scale=SCALE[name], **kw)
    assert limits_ordered(t)
    return t, {n: np.ascontiguousarray(a[:, 1]) for n, a in t.items()}


def dict_of(params, table, b):
    """the parameter dict trajectory b plans under"""
    return params_of(params, table, b, 1)


class FdCase(Case):
    """tests/test_gpu_policy_rollout.py's Case with the FULL_DDP setting chosen (its CarParking is FULL_DDP = 0)"""

    def __init__(self, ilqg, name, fd, strict=False, groups=0, count=1, batch=B, opts=None):
        self.name = name
        prob, _, st, self.N, self.params, self.opts, self.x0, self.u0 = base.setup(name, batch)
        self.problem, self.fd = prob, fd
        kw = dict(batch=batch, n_hor=self.N, params=self.params, opts=dict(self.opts, max_iter=40, **(opts or {})), strict=strict or st, groups=groups)
        self.solvers = [ilqg.BatchSolver(prob, fd, **kw) for _ in range(count)]
        if groups:
            assert self.solvers[0].groups() == groups
        self.nx, self.nu = self.solvers[0].problem.nx, self.solvers[0].problem.nu


def oracle_stages(lib, N, params, opts, x0, u0):
    """init, calc_derivs, back_pass, every step size's forward pass and line_search of the oracle driver under `params`:
    dict(x, u, cost, rec, fin, l, L, dV0, dV1, alpha_cost, alpha_ok, accept, alpha_idx, new_cost)"""
    from oracle.harness import Driver
    d = Driver(lib, N, params, opts)
    try:
        out = dict(init=d.init(x0, u0))
        out["x"], out["u"] = d.traj(0)
        out["cost"] = d.scalars()["cost"]
        out["derivs"] = d.calc_derivs()
        out["rec"], out["fin"] = d.derivs()
        out["bp_rc"] = d.back_pass()
        out["l"], out["L"] = d.gains()
        s = d.scalars()
        out["dV0"], out["dV1"] = s["dV0"], s["dV1"]
        passes = [d.forward_pass(a) for a in ALPHAS]
        out["alpha_ok"] = np.array([p[0] for p in passes], dtype=np.int32)
        out["alpha_cost"] = np.array([p[1] for p in passes])
        out["accept"] = d.line_search(0)
        out["alpha_idx"] = d.log_linesearch(0)
        out["new_cost"] = d.scalars()["new_cost"]
        return out
    finally:
        d.close()
