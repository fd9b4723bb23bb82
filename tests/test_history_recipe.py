"""The numpy restatement of z that tests/test_gpu_history.py holds the history's accepted entries to, checked without a GPU:
history_cases.z_recipe — dcost = cost - new_cost, expected = -alpha (dV0 + alpha dV1), z = dcost / expected
(line_search.c:42-45) — gives, bit for bit, the dcost and expected the reference build itself (oracle/_ref; the CPU restatement
where the reference sources are absent) leaves behind a line search that accepted a step, from the cost, new_cost, dV0, dV1 and
step index its driver's trace records for that search.  CarParking and almix, FULL_DDP 0 and 1, the searches of the first
iterations one at a time (a solve of max_iter = k ends behind the k-th search).  Passes without the feature: it keeps the GPU
comparison honest."""
import os

import numpy as np
import pytest

from history_cases import DEFAULT_ALPHA, z_recipe
from oracle.harness import CAR_N, CAR_PARAMS, CAR_X0, Driver, almix_case, lib_path


def case(problem):
    if problem == "carparking":
        rng = np.random.default_rng(11)
        return CAR_N, CAR_PARAMS, {}, np.array(CAR_X0), 0.1 * rng.standard_normal((CAR_N, 2))
    params, opts, x0, u0 = almix_case()
    return len(u0), params, opts, x0, u0


@pytest.mark.parametrize("fd", [0, 1])
@pytest.mark.parametrize("problem", ["carparking", "almix"])
def test_z_of_an_accepted_search_is_the_reference_builds(oracle_built, problem, fd):
    lib = lib_path("ref", problem, fd)
    if not os.path.exists(lib):
        lib = lib_path("oracle", problem, fd)
    N, params, opts, x0, u0 = case(problem)
    accepted = rejected = 0
    for k in range(1, 7):
        d = Driver(lib, N, params, dict(opts, max_iter=k))
        assert d.init(x0, u0) == 1
        d.solve()
        sc, tr = d.scalars(), d.trace()
        d.close()
        if len(tr["alpha_idx"]) < k:
            break  # (the solve left before its k-th search)
        idx = int(tr["alpha_idx"][k - 1])
        if idx > len(DEFAULT_ALPHA):
            rejected += 1  # (no step size accepted: the fields keep the last candidate's values, no recipe for them)
            continue
        dcost, expected, z = z_recipe(tr["cost"][k - 1], tr["new_cost"][k - 1], DEFAULT_ALPHA[idx - 1], tr["dV0"][k - 1], tr["dV1"][k - 1])
        assert dcost == sc["dcost"] and expected == sc["expected"], (problem, fd, k, float(dcost), sc["dcost"], float(expected), sc["expected"])
        assert expected > 0 and z == sc["dcost"] / sc["expected"] and z > 0, (problem, fd, k)
        accepted += 1
    assert accepted >= 2, "too few accepted searches to pin the recipe"
    assert problem != "almix" or rejected >= 1  # (almix's first search is rejected: the recipe is not applied to it)
    print("%s fd%d: %d accepted searches hold the recipe bit for bit, %d rejected" % (problem, fd, accepted, rejected))
