"""What tests/test_gpu_lambda_branches.py compares the device's regularisation schedule and gradient exit against, pinned to
the reference's own iLQG() (no GPU): the generator tests/lambda_cases.py gives, from the CPU restatement and — where the
reference build oracle/_ref exists — from that build live, what tests/golden/lambda_schedule.npz records of the reference
build, bit for bit; its plain restatement of the loop reproduces every lambda and integer of every case, sequence and batch
entry, and each of its mutants changes one; every branch the cases were chosen for is there (a condition: nothing is
skipped); and every decision has margin, so that the FMA-contracting builds can be held to the integers exactly."""
import os

import numpy as np
import pytest

import lambda_cases as LC
from conftest import golden
from oracle.harness import lib_path

KINDS = ["oracle"] + (["ref"] if os.path.exists(lib_path("ref", "carparking", 1)) else [])


def test_generator_reproduces_the_golden_bit_for_bit(oracle_built):
    g = golden("lambda_schedule.npz")
    for kind in KINDS:
        out = LC.golden_of(kind)
        assert sorted(out) == sorted(g.files), kind
        for k, v in out.items():
            assert v.dtype == g[k].dtype and np.array_equal(v, g[k]), (kind, k, v, g[k])
    assert os.path.getsize(LC.GOLDEN) <= os.path.getsize(os.path.join(os.path.dirname(LC.GOLDEN), "regtype2.npz"))


def test_restatement_reproduces_every_lambda_of_the_reference(oracle_built):
    runs = LC.all_runs()
    assert len(runs) >= len(LC.CASES) + sum(q[6] for q in LC.SEQS.values())
    for tag, r, lam, dlam in runs:
        s = LC.restated(r, lam, dlam)
        assert LC.agrees(s, r), (tag, s, r)
        # what the restatement adds: dlambda.  Behind a line search it is the factor lambda just moved by
        if len(r["calls"]) and r["ls_lambda"][-1] > r["opts"]["lambdaMin"] and r["status"] == LC.ST_MAX_ITER and r["accepted"][-1]:
            assert r["lam"] == r["ls_lambda"][-1] * s["dlam"], tag


@pytest.mark.parametrize("mutant", LC.MUTANTS)
def test_each_mutant_of_the_restatement_is_caught(oracle_built, mutant):
    caught = [tag for tag, r, lam, dlam in LC.all_runs() if not LC.agrees(LC.restated(r, lam, dlam, mutant), r)]
    print("%s: changes %d of %d runs, first %s" % (mutant, len(caught), len(LC.all_runs()), caught[:3]))
    assert caught, mutant
    # and by a single case or batch entry, which is what the staged device calls run
    assert any(not t.startswith("seq/") for t in caught), mutant


def _facts(c, r):
    """the classes a case's reference run shows"""
    o, e = r["opts"], LC.expected(r, c["lam"], c["dlam"])
    s = LC.restated(r, c["lam"], c["dlam"])
    f, mn, mx, tol = o["lambdaFactor"], o["lambdaMin"], o["lambdaMax"], o["tolGrad"]
    sweeps, last = s["sweep_lambda"], s["sweep_lambda"][-1]
    reached, grad, nodesc = e["status_back"] == LC.ST_ACTIVE, e["status_back"] == LC.ST_CONVERGED_GRAD, e["status_back"] == LC.ST_NO_DESCENT
    n = e["calls_back"]
    out = set()
    out.add("first" if reached and n == 1 else "")
    out.add("entry_above_max" if reached and n == 1 and c["lam"] > mx else "")
    if reached and n > 1:
        out.add("fail%d" % min(n - 1, 6))
    out.add("d_one" if c["dlam"] == 1.0 else "d_low" if c["dlam"] < 1.0 / f else "d_high" if c["dlam"] > 1.0 else "")
    out.add("entry_zero" if c["lam"] == 0.0 and n > 1 and sweeps[1] == mn else "")
    out.add("own_min" if mn != LC.DEFAULTS["lambdaMin"] and n > 1 and sweeps[1] == mn else "")
    if nodesc:
        out |= {"max_exit", "max_first" if n == 1 else "max_middle" if n == 2 else "max_late"}
        assert e["lam_back"] > mx or "known_difference" in c["cls"]
    out.add("tie_max" if mx in sweeps[1:] else "")
    out.add("grad" if grad else "")
    out.add("no_grad" if reached else "")
    if reached:
        out.add("lambda_false" if r["g_norm"] < tol and last > 1e-5 else "")
        out.add("tol_false" if r["g_norm"] > tol and last < 1e-5 else "")
        out.add("tie_lambda" if r["g_norm"] < tol and last == 1e-5 else "")
        out.add("tie_tol" if r["g_norm"] == tol and last < 1e-5 else "")
    if grad:
        out.add("below_tie_lambda" if last == LC.BELOW else "")
        out.add("above_tie_tol" if tol == np.nextafter(r["g_norm"], np.inf) else "")
        out.add("down_above_min" if last > mn and r["lam"] > 0.0 else "down_at_min" if last == mn and r["lam"] == 0.0 else
                "down_below_min" if 0.0 < last < mn and r["lam"] == 0.0 else "down_zero" if last == 0.0 and r["lam"] == 0.0 else "")
        out.add("grad_retry" if n > 1 else "")
    if nodesc and r["lam"] <= mx:  # (the exit took lambda above lambdaMax; the gradient test behind it lowered it again)
        out.add("known_difference")
    out.discard("")
    return out


def test_every_required_branch_is_present(oracle_built):
    seen, pairs = set(), set()
    for name, c in LC.CASES.items():
        have = _facts(c, LC.case_run(name))
        assert set(c["cls"]) <= have, (name, c["cls"], have)
        seen |= set(c["cls"])
        pairs |= {(a, b) for a in c["cls"] for b in c["cls"]}
    assert set(LC.REQUIRED) <= seen, set(LC.REQUIRED) - seen
    assert set(LC.REQUIRED_PAIRS) <= pairs, set(LC.REQUIRED_PAIRS) - pairs
    assert "known_difference" in LC.CASES[LC.KNOWN_DIFFERENCE]["cls"]
    assert set(LC.CASES[n]["problem"] for n in LC.GAINS_OF) == set(c["problem"] for c in LC.CASES.values())


def test_sequences_take_step_4_through_both_directions(oracle_built):
    for name, q in LC.SEQS.items():
        assert 4 <= q[6] <= 8
    # accepted steps: under lambdaMin, then 0; a failing sweep at 0 restarts from lambdaMin
    for name in ("acc_to_zero", "acc_to_zero_syn"):
        r = LC.seq_runs(name)[-1]
        mn, ls = r["opts"]["lambdaMin"], r["ls_lambda"].tolist()
        i = next(i for i, v in enumerate(ls) if 0.0 < v < mn)
        assert r["accepted"][:i + 1].all() and (ls[i + 1] == 0.0 or (ls[i + 1] == mn and r["calls"][i + 1] == 2)), (name, ls)
    r = LC.seq_runs("acc_to_zero_syn")[-1]
    assert np.any((r["calls"] == 2) & (r["ls_lambda"] == r["opts"]["lambdaMin"]))  # (the sweep at 0 failed)
    r = LC.seq_runs("acc_to_zero")[-1]
    assert r["status"] == LC.ST_CONVERGED_GRAD and r["lam"] == 0.0 and r["iterations"] == 5 and LC.SEQS["acc_to_zero"][6] > 6
    # rejected steps: lambdaMin from 0 (second max, arm lambdaMin), lambdaFactor first (first max, that arm), then both
    # other arms, up to the exit
    q = LC.SEQS["rej_from_zero"]
    runs = LC.seq_runs("rej_from_zero")
    r, o = runs[-1], runs[-1]["opts"]
    assert not r["accepted"].any() and r["status"] == LC.ST_LAMBDA_MAX and r["rc"] == 1 and r["iterations"] == len(r["calls"]) - 1 < q[6] - 1
    assert q[4] == 0.0 and q[5] < 1.0 / o["lambdaFactor"] and r["ls_lambda"][1] == o["lambdaMin"] and r["ls_lambda"][2] > o["lambdaMin"] * o["lambdaFactor"]
    assert r["lam"] > o["lambdaMax"] >= r["ls_lambda"][-1]
    for name in ("rej_tie", "rej_syn"):  # the raise onto lambdaMax itself is no exit
        r = LC.seq_runs(name)[-1]
        i = r["ls_lambda"].tolist().index(r["opts"]["lambdaMax"])
        assert i > 0 and not r["accepted"][i - 1], name
    r = LC.seq_runs("rej_tie")[-1]
    assert r["status"] == LC.ST_LAMBDA_MAX and r["ls_lambda"][-1] == r["opts"]["lambdaMax"]


@pytest.mark.parametrize("name", list(LC.BATCHES))
def test_mixed_batches_hold_every_kind_of_lane_side_by_side(oracle_built, name):
    runs = LC.batch_runs(name)
    es = [LC.expected(r, e[1], e[2]) for r, e in zip(runs, LC.BATCHES[name][3])]
    calls = [e["calls_back"] for e in es if e["status_back"] == LC.ST_ACTIVE]
    assert {1, 2, 3, 4} <= set(calls) and max(calls) >= 5, calls
    assert any(e["status_back"] == LC.ST_NO_DESCENT for e in es) and any(e["status_back"] == LC.ST_CONVERGED_GRAD for e in es)
    assert len(set(e[0] for e in LC.BATCHES[name][3])) >= 3  # (more than one start)
    assert len(runs) % 4 != 0 or name != "syn1"  # (the quad kernel's last wavefront is partly filled)


def _sweep_counts(c_or_e, r, lam, dlam, problem, fd, first, kind):
    s = LC.restated(r, lam, dlam)
    return [(w["rc"], int(w["done"].sum())) for w in (LC.sweep_of(problem, fd, first, v, kind) for v in s["sweep_lambda"])]


def test_every_decision_has_margin(oracle_built):
    """The integers of a product (FMA-contracting) build are held exactly, so no decision may hang on a last bit:
    - at every lambda a case or batch entry visits, one back_pass() of its own (regtype2_cases.sweep) fails or completes as
      the loop's did, and the reference built with FMA contraction (lib_path("ref_contract")) gives the same return code
      and the same count of completed steps, from a start it computed itself;
    - the whole run — cases, sequences, batches — gives the same integers and the same lambdas in that build;
    - the gradient test's operands are a factor 10 from each other, but for the ties, which are exact by construction
      (lambda: the constant itself and its neighbour; tolGrad: taken from the build under test)."""
    contract = os.path.exists(lib_path("ref_contract", "carparking", 1))
    assert contract or "ref" not in KINDS, "the reference is here: its contracting builds must be, too (oracle/Makefile CONTRACT_LIBS)"
    singles = [(n, c["problem"], c["fd"], c["first"], c["opts"], c["lam"], c["dlam"]) for n, c in LC.CASES.items()]
    for n, (problem, fd, opts, lst) in LC.BATCHES.items():
        singles += [("%s/%d" % (n, i), problem, fd, e[0], opts, e[1], e[2]) for i, e in enumerate(lst)]
    for tag, problem, fd, first, opts, lam, dlam in singles:
        r = LC.run(problem, fd, first, opts, lam, dlam)
        e = LC.expected(r, lam, dlam)
        counts = _sweep_counts(None, r, lam, dlam, problem, fd, first, "oracle")
        n = e["calls_back"]
        assert len(counts) == n and all(rc == 1 for rc, _ in counts[:-1]) and counts[-1][0] == e["bp_rc_back"], (tag, counts, e["bp_rc_back"])
        if e["bp_rc_back"] == 0:  # the loop's last sweep is that sweep: the gains the GPU tests compare belong to it
            w = LC.sweep_of(problem, fd, first, e["last_sweep_lambda"])
            assert w["g_norm"] == r["g_norm"] and np.array_equal(w["dV"], r["dV"]), tag
            tol = r["opts"]["tolGrad"]
            if opts.get("tolGrad") not in ("g", "g+"):
                assert r["g_norm"] > 10.0 * tol or r["g_norm"] < 0.1 * tol, (tag, r["g_norm"], tol)
            if e["last_sweep_lambda"] not in (1e-5, LC.BELOW):
                assert e["last_sweep_lambda"] > 1.04e-5 or e["last_sweep_lambda"] < 0.96e-5, tag
        for kind in KINDS[1:] + (["ref_contract"] if contract else []):
            assert _sweep_counts(None, r, lam, dlam, problem, fd, first, kind) == counts, (tag, kind)
    if contract:
        for (tag, r, lam, dlam), (_, rc, _, _) in zip(LC.all_runs(), LC.all_runs("ref_contract")):
            for k in ("rc", "iterations", "pending", "status", "lam"):
                assert r[k] == rc[k], (tag, k, r[k], rc[k])
            for k in ("calls", "accepted", "ls_lambda"):
                assert np.array_equal(r[k], rc[k]), (tag, k, r[k], rc[k])
