"""The inputs of tests/test_gpu_solve_stream_rows.py, held by the CPU oracle alone (no GPU): a stream test over them cannot be
vacuous.  For hxtest FULL_DDP 1 (max_iter 60) and almix FULL_DDP 1 (almix_case, max_iter 80) each of the 230 starts is solved
twice by the oracle's driver, under the nominal parameters and under its own rows and windows (tests/stream_rows_cases.py):
every start initialises; the iteration counts take at least 4 distinct values, so a stream of them refills while others
iterate; and the cost under the own rows differs from the nominal one for more than half the starts, so the rows are no
no-op."""
import numpy as np
import pytest

from oracle.harness import lib_path
from stream_rows_cases import TOTAL, Inputs, oracle_solve


@pytest.mark.parametrize("name", ["hxtest", "almix"])
def test_the_starts_finish_at_different_iterations_and_their_rows_matter(oracle_built, name):
    inp = Inputs(name)
    lib = lib_path("oracle", inp.problem, inp.fd)
    own = [oracle_solve(lib, inp, s) for s in range(TOTAL)]
    nominal = [oracle_solve(lib, inp, s, own_rows=False) for s in range(TOTAL)]
    assert all(r["init"] == 1 for r in own) and all(r["init"] == 1 for r in nominal), "a start does not initialise"
    it_own, it_nom = np.array([r["iterations"] for r in own]), np.array([r["iterations"] for r in nominal])
    assert len(np.unique(it_own)) >= 4 and len(np.unique(it_nom)) >= 4, (np.unique(it_own), np.unique(it_nom))
    differ = sum(r["cost"] != q["cost"] for r, q in zip(own, nominal))
    assert differ > TOTAL // 2, differ
    assert inp.steps or name != "almix"
    for t in list(inp.rows.values()) + list(inp.steps.values()):
        assert t.shape[0] == TOTAL and np.all(np.isfinite(t))
