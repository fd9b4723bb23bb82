"""TEST INFRASTRUCTURE — the inputs of the tests of BatchSolver.solve_stream(params=..., param_steps=..., history=...)
(ilqg_batch_solve_stream_rows): tests/test_solve_stream_rows_recipe.py (no GPU: the CPU oracle pins that these inputs make a
stream refill while others iterate and that the rows are no no-op), tests/test_solve_stream_rows_binding.py (no GPU) and
tests/test_gpu_solve_stream_rows.py.

Shapes: B = 70 slots (one full and one partly filled wavefront, as tests/test_gpu_policy_rollout.py), TOTAL = 230 starts,
3.3 batches' worth as in tests/test_gpu_solve.py's stream test.  The rows of the fixed-size parameters are the 5 % draws of
tests/policy_param_cases.py, draws(params, NAMED[name], TOTAL, 2)[:, 1]; a per-time-step name gets value * (1 + 0.05 N(0, 1))
per entry, seed STEP_SEED."""
import numpy as np

from oracle.harness import CAR_PARAMS, HX_N, HX_PARAMS, SYN_PARAMS_TIGHT, almix_case, hx_inputs, syn_inputs
from policy_param_cases import NAMED, PER_STEP, draws

B, TOTAL = 70, 230
STEP_SEED = 61
# name -> (problem, FULL_DDP, strict)
BUILDS = {"carparking": ("carparking", 0, False), "carparking_strict": ("carparking", 0, True), "hxtest": ("hxtest", 1, False),
          "almix": ("almix", 1, False), "almix_strict": ("almix", 1, True), "synth16x8": ("synth16x8", 1, False),
          "carparking_wave": ("carparking", 0, "wave")}


class Inputs:
    """one build's stream: problem, fd, strict, N, params, opts, x0 [total, nx], u0 [total, N, nu], rows {name: [total, size]}
    and steps {name: [total, N + 1]} (empty for a build of the wave mapping's tests without rows)"""

    def __init__(self, name, total=TOTAL):
        self.name, self.total = name, total
        self.problem, self.fd, self.strict = BUILDS[name]
        if self.problem == "carparking":
            from conftest import load_package
            self.N, self.params, self.opts = 500, CAR_PARAMS, dict(max_iter=150)
            self.x0, self.u0 = load_package().synth.car_batch(total, self.N)
        elif self.problem == "hxtest":
            self.N, self.params, self.opts = HX_N, HX_PARAMS, dict(max_iter=60)
            self.x0, self.u0 = hx_inputs(total)
        elif self.problem == "almix":
            self.params, self.opts, self.x0, self.u0 = almix_case(batch=total)
            self.N = self.u0.shape[1]
        elif self.problem == "synth16x8":
            self.N, self.params, self.opts = 40, SYN_PARAMS_TIGHT, dict(max_iter=120)
            self.x0, self.u0 = syn_inputs(total, self.N)
        else:
            raise ValueError(name)
        self.params = {k: np.atleast_1d(np.asarray(v, dtype=np.float64)) for k, v in self.params.items()}
        named = NAMED["carparking" if self.problem == "carparking" else self.problem]
        self.rows = {n: np.ascontiguousarray(t[:, 1]) for n, t in draws(self.params, named, total, 2).items()}
        self.steps = {}
        if self.problem in PER_STEP:
            n = PER_STEP[self.problem]
            rng = np.random.default_rng(STEP_SEED)
            self.steps[n] = self.params[n][None, :] * (1.0 + 0.05 * rng.standard_normal((total, self.N + 1)))

    def params_of(self, s):
        """the parameter dict start s plans under: the nominal one with its rows and windows"""
        out = dict(self.params)
        out.update({n: t[s].copy() for n, t in self.rows.items()})
        out.update({n: t[s].copy() for n, t in self.steps.items()})
        return out

    def nominal_rows(self):
        return {n: np.ascontiguousarray(np.broadcast_to(self.params[n], (self.total, self.params[n].size))) for n in self.rows}


def oracle_solve(lib, inp, s, own_rows=True, trace=False):
    """start s of `inp` solved by the CPU driver under its own parameter dict (or the nominal one): dict of init (drv_init's
    return value), cost, iterations and, if asked for, the driver's trace"""
    from oracle.harness import Driver
    d = Driver(lib, inp.N, inp.params_of(s) if own_rows else inp.params, inp.opts)
    try:
        out = dict(init=d.init(inp.x0[s], inp.u0[s]))
        if out["init"] == 1:
            d.solve()
            sc = d.scalars()
            out.update(cost=sc["cost"], iterations=int(sc["iterations"]))
            if trace:
                out["trace"] = d.trace()
        return out
    finally:
        d.close()
