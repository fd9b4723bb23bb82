"""The forms the generated file emits for batched back-ends only — the factored tensor tables with bp_tensor_basis,
ilqg_step_part, ilqg_deriv_prepare / ilqg_deriv_part — called on the host (oracle/driver.c behind DRV_FUNC_IN_UNIT, the
'*_forms' builds of oracle/Makefile; no GPU) and held
  - to the derivatives of the problem's definition (tests/deriv_cases.py) at the bar of tests/test_deriv_cases_recipe.py,
    four times the reference build's measured error for the problem, and
  - to calc_derivs() / forward_pass() of the same build bit for bit, where the generator's docstrings promise the same bits
    (the builds are FMA-free);
and absent exactly where the generator's docstrings exclude the problem (multipliers; for the parts of the derivative
record also limits that depend on the state, and tensors that do not factor)."""
import os

import numpy as np
import pytest

import deriv_cases as DC
from conftest import golden
from oracle.harness import lib_path

KINDS = ["oracle_forms"] + (["ref_forms"] if os.path.exists(lib_path("ref_forms", "carparking", 1)) else [])
BAR_FACTOR = 4.0
# what tools/gen_problem.py's docstrings say (_emit_factored_tensors, _emit_step_parts, _emit_deriv_parts)
EXPECTED = dict(carparking={"step_parts"}, hxtest={"step_parts"}, almix=set(), brachi=set(), brachi_hli=set(),
                synth10hx={"step_parts", "factored_tensors"}, synth16p={"step_parts"},
                synth16x8={"step_parts", "factored_tensors", "deriv_parts"})
FIRST_ORDER = ("cx", "cxx", "cu", "cuu", "cxu", "fx", "fu", "lower", "upper")


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", [n for n in DC.CASES if n != "almix_b"])
def test_forms_for_batched_back_ends(oracle_built, name, kind):
    problem, _, _, _, _, steps = DC._case(name)
    D, t = DC.definition(problem), DC.case_truth(name)
    n, m = D.n, D.m
    g = golden("deriv_truth.npz")
    bar = BAR_FACTOR * float(g[DC.key_of(name, 1)])
    d, xs, us = DC.swept_driver(name, 1, kind, (t["xs"], t["us"]))
    assert d.forms() == EXPECTED[problem], (problem, d.forms())

    if "step_parts" in d.forms():
        # "c = term[0]; c = c + term[1]; ... reproduces ddpL's t->c to the last bit", the dynamics' assignments unchanged
        nxt, cost = d.step_parts()
        assert np.array_equal(nxt, xs[1:]) and np.array_equal(cost, d.step_costs(0)[:-1])
        eps = np.finfo(float).eps
        assert np.all(np.abs(nxt - t["next"]) <= 64 * eps * np.abs(t["next"]).max(axis=1, keepdims=True))
        assert np.all(np.abs(cost - t["cost"][:-1]) <= 64 * eps * np.abs(t["cost"][:-1]))

    parts = None
    if "deriv_parts" in d.forms():  # (in front of calc_derivs: what the records hold then is the parts' alone)
        assert d.deriv_parts() == 1
        parts = d.derivs()[0][list(steps)]
    assert d.calc_derivs() == 1
    rec = d.derivs()[0][list(steps)]
    have = DC.split(rec, n, m, 1)

    if "factored_tensors" in d.forms():
        ten, basis = d.factored_tensors()
        ten, basis = ten[list(steps)], basis[list(steps)]
        stored = np.concatenate([have["fxx"], have["fuu"], have["fxu"]], axis=1)
        assert np.array_equal(ten, stored)  # "t->fxx[...] == coef * basis[slice]"
        e = DC.error(DC.join(dict(have, fxx=ten[:, :n * DC.tri(n)], fuu=ten[:, n * DC.tri(n):n * (DC.tri(n) + DC.tri(m))],
                                  fxu=ten[:, n * (DC.tri(n) + DC.tri(m)):]), n, m, 1), t["rec"], n, m, 1, only=("fxx", "fuu", "fxu"))
        want = g["%s/products" % name]
        ep = float((np.abs(basis - want).max(axis=1) / np.abs(want).max(axis=1)).max())
        print("%s %s: factored tensors %.3g, products %.3g (bar %.3g)" % (name, kind, e, ep, bar))
        assert e <= bar and ep <= bar, (e, ep, bar)
    else:
        assert "%s/products" % name not in g.files

    if parts is not None:
        got = DC.split(parts, n, m, 1)
        for k in FIRST_ORDER:  # "by the expression of the function it comes from ... the FMA-free build gives the same bits"
            assert np.array_equal(got[k], have[k]), k
        nb = basis.shape[1]
        assert np.array_equal(got["fxx"][:, :nb], basis)
        e = DC.error(parts, t["rec"], n, m, 1, only=FIRST_ORDER)
        print("%s %s: record in parts %.3g (bar %.3g)" % (name, kind, e, bar))
        assert e <= bar
    d.close()
