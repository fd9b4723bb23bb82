"""TEST INFRASTRUCTURE — the cases of BatchSolver.set_param_steps_batch (a window of a per-time-step parameter per trajectory),
for tests/test_param_steps_recipe.py (no GPU: what the GPU tests compare against exists and is no no-op) and
tests/test_gpu_param_steps.py.

Problems: almix (oracle/harness.py almix_case, N = 80; `vref` feeds the running constraint hle) and brachi_hli
(brachi_hli_case(n=64), every slot the case's one start; `ymin` feeds hli at every step and hfe at k = n_hor: the only case
that reads the final index, and its slots differ only through the rows).  B = 70 (one full and one partly filled wavefront),
compared slots 0, 63, 64, 69.  Rows: row[b][k] = nominal[k] (1 + 0.05 N(0, 1)) element by element, default_rng(53): every
(b, k) is distinct, so a transposed or mis-strided table shows."""
import numpy as np

from oracle.harness import almix_case, brachi_hli_case
from params_batch_cases import oracle_stages  # noqa: F401 (the stages of the oracle driver, shared)

B = 70
SLOTS = (0, 63, 64, 69)
STEP_NAME = dict(almix="vref", brachi_hli="ymin")
BRACHI_N = 64
# (problem, FULL_DDP, FMA-free) of the GPU comparison against the oracle; on the CPU both FULL_DDP settings of both problems
BUILDS = [("almix", 1, False), ("almix", 1, True), ("brachi_hli", 0, False), ("brachi_hli", 1, False)]
CPU_BUILDS = [("almix", 0), ("almix", 1), ("brachi_hli", 0), ("brachi_hli", 1)]


def setup(name, batch=B, n=None):
    """(n_hor, params, opts, x0 [batch, nx], u0 [batch, N, nu])"""
    if name == "almix":
        params, opts, x0, u0 = almix_case(batch=batch)
        return u0.shape[1], params, opts, x0, u0
    if name == "brachi_hli":
        params, opts, x0, u0 = brachi_hli_case(n or BRACHI_N)
        return len(u0), params, opts, np.ascontiguousarray(np.tile(x0, (batch, 1))), np.ascontiguousarray(np.tile(u0, (batch, 1, 1)))
    raise ValueError(name)


def step_rows(name, params, batch=B):
    """[batch, n_hor + 1]: trajectory b's window of the problem's per-time-step parameter"""
    nominal = np.asarray(params[STEP_NAME[name]], dtype=np.float64)
    rng = np.random.default_rng(53)
    return np.ascontiguousarray(nominal[None, :] * (1.0 + 0.05 * rng.standard_normal((batch, nominal.size))))


def dict_of(name, params, rows, b):
    """the parameter dict trajectory b plans under"""
    return dict(params, **{STEP_NAME[name]: rows[b]})


class StepCase:
    """`count` solvers of one build on the case's inputs"""

    def __init__(self, ilqg, name, fd, strict=False, count=1, groups=0, batch=B, opts=None, n=None):
        self.name, self.problem, self.fd, self.step = name, name, fd, STEP_NAME[name]
        self.N, self.params, self.opts, self.x0, self.u0 = setup(name, batch, n)
        kw = dict(batch=batch, n_hor=self.N, params=self.params, opts=dict(self.opts, max_iter=40, **(opts or {})), strict=strict, groups=groups)
        self.solvers = [ilqg.BatchSolver(name, fd, **kw) for _ in range(count)]
        if groups:
            assert self.solvers[0].groups() == groups
        self.rows = step_rows(name, self.params, batch)

    def close(self):
        for s in self.solvers:
            s.close()
