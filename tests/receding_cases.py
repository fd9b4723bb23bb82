"""TEST INFRASTRUCTURE — the receding-horizon chain the fixtures tests/golden/receding_*.npz record and the tests replay:
solve cold, shift the plan by s steps with the last control held, restart from the plan's own x[s] (what a caller of the
reference's MEX entry does between two calls: u_nom = [u(:, s+1:end), tail] and the new x0, iLQG_mex.c:113-120), and
solve warm.  Used by tests/golden/make_receding_goldens.py, tests/test_receding_golden.py and tests/test_gpu_receding.py."""
import numpy as np

from conftest import load_package
from oracle.harness import (CAR_PARAMS, HX_N, HX_PARAMS, SYN_PARAMS_TIGHT, Driver, almix_case, hx_inputs, syn_inputs)


def case(name, batch=3):
    """dict(problem, fd, n, s, params, opts, x0 [batch, nx], u0 [batch, n, nu]) of a fixture's problem with `batch` starts"""
    if name == "carparking":
        x0, u0 = load_package().synth.car_batch(batch, 500)
        return dict(problem="carparking", fd=0, n=500, s=10, params=CAR_PARAMS, opts=dict(max_iter=400), x0=x0, u0=u0)
    if name == "hxtest":
        x0, u0 = hx_inputs(batch)
        return dict(problem="hxtest", fd=1, n=HX_N, s=5, params=HX_PARAMS, opts=dict(max_iter=60), x0=x0, u0=u0)
    if name == "synth16x8":
        x0, u0 = syn_inputs(batch, 60)
        return dict(problem="synth16x8", fd=1, n=60, s=5, params=SYN_PARAMS_TIGHT, opts=dict(max_iter=200), x0=x0, u0=u0)
    if name == "almix":  # its per-time-step parameter vref is NOT shifted: the same window for both solves
        params, opts, x0, u0 = almix_case(batch=batch)
        return dict(problem="almix", fd=1, n=u0.shape[1], s=4, params=params, opts=opts, x0=x0, u0=u0)
    raise ValueError(name)


CASES = ("carparking", "hxtest", "synth16x8", "almix")


def shift_plan(x, u, s):
    """(x0', u') of a plan shifted by s steps, the last control held"""
    return x[s].copy(), np.concatenate([u[s:], np.repeat(u[-1:], s, axis=0)])


def chain(lib, c):
    """the chain through one driver build (reference, oracle), one trajectory at a time: {key: array [batch, ...]}"""
    out = {k: [] for k in ("plan_x", "plan_u", "plan_cost", "plan_iters", "plan_rc", "shift_x0", "shift_u", "init_ok", "init_x",
                           "init_u", "init_cost", "warm_cost", "warm_iters", "warm_rc")}
    for b in range(len(c["x0"])):
        d = Driver(lib, c["n"], c["params"], c["opts"])
        assert d.init(c["x0"][b], c["u0"][b]) == 1
        out["plan_rc"].append(d.solve())
        x, u = d.traj(0)
        sc = d.scalars()
        out["plan_x"].append(x), out["plan_u"].append(u), out["plan_cost"].append(sc["cost"]), out["plan_iters"].append(sc["iterations"])
        d.close()
        x0s, us = shift_plan(x, u, c["s"])
        out["shift_x0"].append(x0s), out["shift_u"].append(us)
        d = Driver(lib, c["n"], c["params"], c["opts"])  # a new call of the MEX entry
        out["init_ok"].append(d.init(x0s, us))
        xi, ui = d.traj(0)
        out["init_x"].append(xi), out["init_u"].append(ui), out["init_cost"].append(d.scalars()["cost"])
        out["warm_rc"].append(d.solve())
        sc = d.scalars()
        out["warm_cost"].append(sc["cost"]), out["warm_iters"].append(sc["iterations"])
        d.close()
    return {k: np.asarray(v) for k, v in out.items()}
