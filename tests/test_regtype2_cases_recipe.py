"""What tests/test_gpu_regtype2.py compares the device's regType-2 sweeps against, pinned to the reference's own sources (no
GPU): on every line of tests/regtype2_cases.py's TABLE the CPU restatement gives what tests/golden/regtype2.npz records of
the reference build — start state, rc, value changes, gradient norm, completed steps and their gains, bit for bit — and,
where the reference build oracle/_ref exists, what that build gives live.  The table's own columns (rc, completed steps)
and the three conditions its grids were chosen for are asserted on the same numbers."""
import os

import numpy as np
import pytest

import regtype2_cases as R
from conftest import golden
from oracle.harness import lib_path

CASES = [(p, fd) for p in R.PROBLEMS for fd in (0, 1)]


def test_table_covers_every_case_once():
    assert sorted(set((t[0], t[1]) for t in R.TABLE)) == sorted(CASES)
    assert len(set((t[0], t[1], t[4]) for t in R.TABLE)) == len(R.TABLE)
    for p, fd in CASES:
        assert R.lambdas(p, fd)[0] == 0.0  # (regType 2 at lambda = 0 is regType 1 at lambda = 0: the GPU tests' part d)
        assert set(t[2] for t in R.table(p, fd)) == {"it3" if (p, fd) in R.IT3 else "roll"}


def test_bars_other_than_the_tolerance_are_ten_fma_differences_of_the_reference():
    """a line whose bar is not the single-pass tolerance: 10 times the distance between the reference's own sources built
    with and without FMA contraction on that line — oracle/Makefile's `_contract` build: the flags of the reference build
    with -mfma -ffp-contract=fast in place of -ffp-contract=off and no -march=native, so that the host does not enter (with
    -march=native the figure was 2.99e-10 on one host and 5.13e-10 on another).  The table carries the figure of gcc 11.4;
    which multiply-adds a compiler contracts is its own choice, so where the build exists the figure is held within a
    factor of 2 of the table's, not to its digits."""
    special = [t for t in R.TABLE if t[7] is not None]
    assert [(t[0], t[1], t[4]) for t in special] == [("synth10hx", 1, 1e4)]
    for problem, fd, _, _, lam, rc, _, bar in special:
        assert rc == 0 and R.TOL < bar <= 1e-8
        if os.path.exists(lib_path("ref_contract", problem, fd)) and os.path.exists(lib_path("ref", problem, fd)):
            far = R.fma_distance(problem, fd, lam)
            print("%s fd%d lambda %g: FMA contraction moves the reference by %.3g; bar %.3g" % (problem, fd, lam, far, bar))
            assert 0.5 * bar <= 10.0 * far <= 2.0 * bar, (far, bar)


@pytest.mark.parametrize("problem,fd", CASES)
def test_oracle_gives_the_reference_builds_bits(oracle_built, problem, fd):
    g = golden("regtype2.npz")
    live = os.path.exists(lib_path("ref", problem, fd))
    s = R.start(problem, fd)
    tag = "%s_fd%d/" % (problem, fd)
    assert np.array_equal(s["x"], g[tag + "x"]) and np.array_equal(s["u"], g[tag + "u"]) and s["cost"] == float(g[tag + "cost"])
    if live:
        sr = R.start(problem, fd, kind="ref")
        for k in ("x", "u", "cost", "rec", "fin"):  # (and the records the device sweeps are fed)
            assert np.array_equal(s[k], sr[k]), k
    for _, _, which, n, lam, rc, ndone, bar in R.table(problem, fd):
        r = R.sweep(problem, fd, lam)
        t = tag + "%g/" % lam
        assert s["n_hor"] == n and s["kind"] == which
        assert r["rc"] == rc == int(g[t + "rc"]) and int(r["done"].sum()) == ndone, (lam, r["rc"], int(r["done"].sum()))
        assert np.array_equal(r["done"], g[t + "done"])
        assert np.array_equal(r["l"][r["done"]], g[t + "l"]) and np.array_equal(r["L"][r["done"]], g[t + "L"]), lam
        assert np.array_equal(r["dV"], g[t + "dV"]) and r["g_norm"] == float(g[t + "g_norm"]), lam
        if live:
            rr = R.sweep(problem, fd, lam, kind="ref")
            assert rr["rc"] == r["rc"] and np.array_equal(rr["done"], r["done"])
            assert np.array_equal(rr["l"][rr["done"]], r["l"][r["done"]]) and np.array_equal(rr["L"][rr["done"]], r["L"][r["done"]]), lam
            assert np.array_equal(rr["dV"], r["dV"]) and rr["g_norm"] == r["g_norm"], lam


@pytest.mark.parametrize("problem,fd", CASES)
def test_grids_meet_their_conditions(oracle_built, problem, fd):
    rows = R.table(problem, fd)
    completed = [t for t in rows if t[4] > 0 and t[5] == 0]
    assert len(completed) >= 2
    assert all(t[6] == t[3] for t in rows if t[5] == 0) and all(t[6] < t[3] for t in rows if t[5] != 0)
    if (problem, fd) in R.IT3:
        assert any(t[4] > 0 and t[5] == 1 and t[6] >= 1 for t in rows)
    for t in completed:
        lam, bar = t[4], (R.TOL if t[7] is None else t[7])
        r2, r1 = R.sweep(problem, fd, lam, 2), R.sweep(problem, fd, lam, 1)
        assert r1["rc"] == 0
        far = max(R.distance(r2["l"], r1["l"]), R.distance(r2["L"], r1["L"]))
        print("%s fd%d lambda %g: regType-2 gains %.3g from the regType-1 ones (%.3g bars)" % (problem, fd, lam, far, far / bar))
        assert far >= 1e4 * bar, (lam, far)
    # lambda = 0: both regularisations add nothing
    r2, r1 = R.sweep(problem, fd, 0.0, 2), R.sweep(problem, fd, 0.0, 1)
    assert r2["rc"] == r1["rc"] and np.array_equal(r2["done"], r1["done"])
    assert np.array_equal(r2["l"][r2["done"]], r1["l"][r1["done"]]) and np.array_equal(r2["L"][r2["done"]], r1["L"][r1["done"]])


@pytest.mark.parametrize("problem,fd", sorted(R.SOLVE_STARTS))
def test_solve_starts_are_the_references_stable_ones(oracle_built, problem, fd):
    """the starts of the free-running solves: the first five (hxtest: the one) of the candidates at which the reference's
    own costs do not move (by SOLVE_STABLE, four orders below the 1e-8 the solves are compared at) under
    one-unit-in-the-last-place changes of the initial controls; the candidates passed over do"""
    chosen = R.SOLVE_STARTS[(problem, fd)]
    assert max(chosen) < R.SOLVE_CANDIDATES and len(chosen) == (1 if problem == "hxtest" else 5)
    for f in range(max(chosen) + 1):
        s = R.solve_sensitivity(problem, fd, f)
        assert (s < R.SOLVE_STABLE) == (f in chosen), (f, s)
    exits = [(int(R.solve(problem, fd, f)[1]["iterations"]), R.solve(problem, fd, f)[0]) for f in chosen]
    print(problem, fd, "(iterations, return value) of the chosen starts:", exits)
    if fd == 0:
        assert all(e[0] == R.SOLVE_ITERS for e in exits) or problem == "hxtest"
    else:  # start 0: every sweep abandoned until lambda > lambdaMax, no iteration done (iLQG.c:273-275)
        rc, sc, tr = R.solve(problem, fd, 0)
        assert int(sc["iterations"]) == 0 and len(tr["alpha_idx"]) == 0 and sc["lambda"] > 1e10
    if os.path.exists(lib_path("ref", problem, fd)):
        for f in chosen:
            (rc, sc, tr), (rc2, sc2, tr2) = R.solve(problem, fd, f), R.solve(problem, fd, f, kind="ref")
            assert rc == rc2 and sc == sc2 and all(np.array_equal(tr[k], tr2[k]) for k in tr)
