"""The derivative records of every generated problem against derivatives taken from its DEFINITION alone (no GPU):
tests/deriv_cases.py differentiates problems/defs/*.py numerically in 80-digit arithmetic — no Deriver, no Emitter, no
printer, no sympy.diff — and here the records of the CPU restatement and, where it exists, of the reference build
(calc_derivs() of the generated pair, the parity target of every kernel) are held to it, per entry, normalised by the size of
the entry's own array at its step.  forward_pass is held to the definition on the way: the roll-out's x[k+1] and the step
costs are the definition's f and augmented L, F at the points.

The bar of a build is FOUR TIMES the reference build's measured worst normalised error for the same problem (deterministic
on the CPU; tests/golden/deriv_truth.npz carries the figures, the truth, the points, parameters, multipliers and weights).
Measured (reference build and CPU restatement alike):

    carparking   FULL_DDP 0  2.3e-16     FULL_DDP 1  7.4e-15  (fxx)
    hxtest                0  1.8e-16              1  2.2e-16
    almix, almix_b        0  2.2e-16              1  2.2e-16
    brachi                                        1  1.8e-14  (cuu)
    brachi_hli            0  1.8e-14  (cuu)       1  1.8e-14  (cuu)
    synth10hx             0  1.9e-16              1  2.9e-16
    synth16x8             0  1.7e-16              1  4.0e-16
    synth16p                                      1  4.0e-16

None is above 1e-13, the size from which a figure would have to be explained from the expression; the array named is where
the worst entry of the two above 1e-15 lies (CarParking: the tensors alone, its FULL_DDP = 0 record is at 2.3e-16; the
Brachistochrone's cost 2 (sqrt(-y - dy dx) - sqrt(-y)) / (-dy) is a difference of square roots, differentiated twice in dy).
No record disagrees with its definition: no generator or definition bug was found, nothing was regenerated.

The differentiator's own error is measured here against the closed-form derivatives of a hand-written function."""
import os

import numpy as np
import pytest

import deriv_cases as DC
from conftest import golden
from oracle.harness import lib_path

KINDS = ["oracle"] + (["ref"] if os.path.exists(lib_path("ref", "carparking", 1)) else [])
BAR_FACTOR = 4.0
MUTANT_MISS = 1e4


def test_differentiator_error_on_a_function_with_closed_form_derivatives():
    """g = sin(a) exp(b) + a^2 b^3 / c, derivatives written out by hand"""
    import mpmath as mp
    mp.mp.dps = DC.DPS
    z = [mp.mpf("0.7"), mp.mpf("-1.3"), mp.mpf("2.1")]
    a, b, c = z
    sa, ca, eb = mp.sin(a), mp.cos(a), mp.exp(b)
    g = lambda w: [mp.sin(w[0]) * mp.exp(w[1]) + w[0]**2 * w[1]**3 / w[2]]
    grad = [ca * eb + 2 * a * b**3 / c, sa * eb + 3 * a**2 * b**2 / c, -a**2 * b**3 / c**2]
    hess = [[-sa * eb + 2 * b**3 / c, ca * eb + 6 * a * b**2 / c, -2 * a * b**3 / c**2],
            [None, sa * eb + 6 * a**2 * b / c, -3 * a**2 * b**2 / c**2],
            [None, None, 2 * a**2 * b**3 / c**3]]
    J, Hs = DC.jacobian(g, z), DC.hessian(g, z)
    scale = abs(g(z)[0])
    worst = max([abs(J[i][0] - grad[i]) / scale for i in range(3)] + [abs(Hs[i][j][0] - hess[i][j]) / scale for i in range(3) for j in range(i, 3)])
    print("differentiator: worst error %.3g of the function's scale" % float(worst))
    assert worst < DC.DIFF_ERROR and worst < 1e-28, float(worst)  # (measured 2.2e-31; deriv_cases.py states it)
    # a structural zero is zero: g does not depend on a fourth variable, and is linear in a fifth
    g2 = lambda w: [g(w)[0] + 3 * w[4]]
    z2 = z + [mp.mpf("0.4"), mp.mpf("0.9")]
    H2 = DC.hessian(g2, z2)
    assert all(H2[3][j][0] == 0 for j in range(5)) and all(H2[4][j][0] == 0 for j in range(5)) and DC.jacobian(g2, z2)[3][0] == 0


@pytest.mark.parametrize("name", DC.CASES)
def test_cases_are_what_they_were_chosen_for(oracle_built, name):
    seen, final = DC.check_case(name)
    if name in ("almix", "almix_b"):
        assert seen.shape == (DC.N_HOR, 2) and (final[0] < 0) == (name == "almix")
    if name == "brachi_hli":
        assert seen.shape == (DC.N_HOR, 1)
    el, fin = DC.multipliers_of(name)
    assert np.all(el != 0.0) and np.all(fin != 0.0)


def test_the_fourteen_builds_are_covered():
    builds = {(DC._case(n)[0], fd) for n, fd in DC.BUILDS}
    assert builds == {("carparking", 0), ("carparking", 1), ("hxtest", 0), ("hxtest", 1), ("almix", 0), ("almix", 1), ("brachi", 1),
                      ("brachi_hli", 0), ("brachi_hli", 1), ("synth10hx", 0), ("synth10hx", 1), ("synth16x8", 0), ("synth16x8", 1),
                      ("synth16p", 1)}


@pytest.mark.parametrize("name,fd", DC.BUILDS)
def test_records_equal_derivatives_of_the_definition(oracle_built, name, fd):
    g = golden("deriv_truth.npz")
    ref = float(g[DC.key_of(name, fd)])
    assert 0.0 < ref < 1e-13, (name, fd, ref)  # (above: a finding to be explained from the expression, not a bar)
    t = DC.case_truth(name)
    for kind in KINDS:
        r = DC.records(name, fd, kind)
        # the point is the right one, and forward_pass computes the definition: the build's own roll-out and its costs under
        # these multipliers and weights are f and the augmented L, F (correctly rounded here; a cost is a sum of a few dozen
        # rounded terms of one sign or nearly so: 64 ulp of the result is generous and far below any wrong term)
        assert np.array_equal(r["xs"], t["xs"]) and np.array_equal(r["us"], t["us"]), (kind, "roll-out")
        eps = np.finfo(float).eps
        assert np.all(np.abs(r["xs"][1:] - t["next"]) <= 64 * eps * np.abs(t["next"]).max(axis=1, keepdims=True)), kind
        assert np.all(np.abs(r["step_costs"] - t["cost"]) <= 64 * eps * np.abs(t["cost"])), (kind, r["step_costs"], t["cost"])
        e = DC.build_error(name, fd, kind)
        print("%s FULL_DDP %d %s: %.3g (reference build %.3g)" % (name, fd, kind, e, ref))
        assert e <= BAR_FACTOR * ref, (name, fd, kind, e, ref)
        if kind == "ref":
            assert e == ref, (name, fd, e, ref)


def test_golden_file_is_what_the_cases_module_computes(oracle_built):
    g = golden("deriv_truth.npz")
    out = DC.golden_of(KINDS[-1])
    assert sorted(out) == sorted(g.files)
    for k, v in out.items():
        if k.endswith("ref_error") and KINDS[-1] != "ref":
            continue  # (the reference build's figures: reproduced where that build exists)
        assert v.dtype == g[k].dtype == np.float64 and np.array_equal(v, g[k]), k
    assert os.path.getsize(DC.GOLDEN) <= max(os.path.getsize(os.path.join(os.path.dirname(DC.GOLDEN), f)) for f in os.listdir(os.path.dirname(DC.GOLDEN))
                                             if f != os.path.basename(DC.GOLDEN))


@pytest.mark.parametrize("mutant", DC.MUTANTS)
def test_each_mutant_misses_its_bar(oracle_built, mutant):
    g = golden("deriv_truth.npz")
    missed = {}
    for name in DC.CASES:
        if name in ("synth16x8", "synth16p") and mutant in ("chain_term_dropped", "branches_exchanged", "w_pen_f_running", "vref_next"):
            continue  # (nothing there for these to touch; spares the n = 16 truth a second evaluation)
        m = DC.mutated(name, mutant)
        if m is None:
            continue
        D, t = DC.definition(DC._case(name)[0]), DC.case_truth(name)
        bar = BAR_FACTOR * float(g[DC.key_of(name, 1)])
        e = max(DC.error(m[0], t["rec"], D.n, D.m, 1), DC.error(m[1], t["fin"], D.n, D.m, 1, final=True))
        missed[name] = e / bar
    print("%s: misses the bar by %s" % (mutant, {k: "%.3g" % v for k, v in missed.items()}))
    assert missed and max(missed.values()) >= MUTANT_MISS, (mutant, missed)
