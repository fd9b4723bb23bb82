"""What tests/test_gpu_linesearch_branches.py compares the device's line searches against, pinned to the reference's own
line_search() (no GPU): on every case of tests/linesearch_cases.py the CPU restatement gives what tests/golden/linesearch.npz
records of the reference build — roll-outs per step size, index, return value, what the scan leaves behind and the candidate
trajectory, bit for bit — and, where the reference build oracle/_ref exists, what that build gives live.  The table's own
conditions (margins of z and of the failures, every class populated as labelled) are asserted on the same numbers, and a
restatement of the scan with switchable mistakes shows that each of them is caught by at least one case."""
import os

import numpy as np
import pytest

import linesearch_cases as LS
from conftest import golden
from oracle.harness import lib_path

NAMES = list(LS.BATCHES)
GOLDEN_FIELDS = ("cost", "dV0", "dV1", "ok", "ac", "idx", "ret", "new_cost", "dcost", "expected", "xc", "uc")


def same(a, b):
    return np.array_equal(a, b, equal_nan=True)  # (NaN: the fields that are not compared, see LS.reference)


@pytest.mark.parametrize("name", NAMES)
def test_oracle_gives_the_reference_builds_bits(oracle_built, name):
    g = golden("linesearch.npz")
    r = LS.reference(name)
    for k in GOLDEN_FIELDS:
        assert same(r[k], g[name + "/" + k]), (name, k)
    if os.path.exists(lib_path("ref", LS.BATCHES[name][0], 0)):
        live = LS.reference(name, "ref")
        for k in LS.FIELDS:
            assert same(r[k], live[k]), (name, k)


@pytest.mark.parametrize("name", NAMES)
def test_table_meets_its_conditions(oracle_built, name):
    r = LS.reference(name)
    alpha, zmin = LS.BATCHES[name][2], LS.BATCHES[name][3]
    A, B = len(alpha), len(r["cls"])
    # margins of the failures: 1 % beyond the limit where a roll-out fails (and 1 % inside in front of that step), 1 % inside where not
    assert np.all(np.where(r["ok"] == 1, r["margin"] >= 0.01, r["margin"] <= -0.01)) and np.all(r["margin_front"] >= 0.01)
    # margins of every z the scan computes, and of every expected reduction it finds negative
    ties = 0
    for b in range(B):
        for i in range(r["idx"][b] if r["ret"][b] else A):
            if not r["ok"][b, i]:
                continue
            dcost = r["cost"][b] - r["ac"][b, i]
            expected = -alpha[i] * (r["dV0"][b] + alpha[i] * r["dV1"][b])
            if expected > 0:
                z = dcost / expected
                if r["tie"][b] and z == zmin:
                    ties += 1
                    continue
                assert abs(z - zmin) >= LS.Z_MARGIN * max(1.0, abs(z)), (name, b, i, z)
            else:
                assert expected == 0.0 or expected <= -LS.Z_MARGIN, (name, b, i, expected)
    assert ties == int(r["tie"].sum())
    # every class: at least two cases, and what its label says
    by = {}
    for b, c in enumerate(r["cls"]):
        by.setdefault(c, []).append(b)
    assert set(by) == set(LS.BATCHES[name][4])
    for c, bs in by.items():
        assert len(bs) >= 2, c
        ok, idx, ret = r["ok"][bs], r["idx"][bs], r["ret"][bs]
        first_ok = np.array([int(np.argmax(o)) if o.any() else A for o in ok])
        if c == "accept0":
            assert np.all(idx == 1) and np.all(ret == 1)
        elif c == "accept_later":
            assert np.all(ret == 1) and np.all(idx > 1) and np.all(ok == 1)
            if A == 8:
                assert set(idx) == set(range(2, 9))  # the last of a first stage and the first of a second for ls_split 1, 3, 4; the last
        elif c == "prefix_accept":
            assert np.all(ret == 1) and np.all(first_ok >= 1) and np.all(idx >= first_ok + 1)
            if A == 8 and name != "brachi6":
                assert {1, 3} <= set(first_ok) and np.any(idx == first_ok + 1) and np.any(idx >= first_ok + 3)
        elif c == "fail_behind_finite":  # finite and rejected, failed, ..., accepted
            assert np.all(ret == 1) and np.all(ok[:, 0] == 1) and np.all(ok[:, 1] == 0) and np.all(idx >= 3) and np.any(idx >= 4)
        elif c == "end_on_failed":
            assert np.all(ret == 0) and np.all(ok[:, 0] == 1) and np.all(ok[:, -1] == 0)
            assert not r["cmp_new_cost"][bs].any() and r["cmp_dexp"][bs].all()
        elif c == "all_fail":
            assert not ok.any() and np.all(idx == A + 1) and np.all(ret == 0) and not r["cmp_dexp"][bs].any() and not r["cmp_new_cost"][bs].any()
        elif c == "neg_expected":
            assert np.all(ret == 0) and np.all(r["dV0"][bs] > 0) and np.all(r["expected"][bs] < 0)
            assert np.all(r["dcost"][bs] < 0)  # (z = dcost / expected would be positive: accepted without the guard)
        elif c == "zero_expected":
            assert np.all(ret == 0) and np.all(r["expected"][bs] == 0.0) and np.all(r["dcost"][bs] > 0)
        elif c == "all_rejected":
            assert np.all(ret == 0) and np.all(idx == A + 1) and ok.any(axis=1).all()
        elif c == "z_above":
            assert zmin == 0.5 and np.all(ret == 1) and len(set(idx)) >= 3
        elif c == "z_below":
            assert zmin == 0.5 and np.all(ret == 0) and np.all(r["dcost"][bs] > 0)  # (zMin = 0 would have accepted)
        elif c == "z_tie":
            assert np.all(r["tie"][bs] == 1) and np.all(idx == 2) and np.all(ret == 1)
        else:
            raise AssertionError(c)
    # what is left out of the comparisons, and nothing else: new_cost behind a failed last roll-out, dcost / expected behind failures only
    for b in range(B):
        tried = r["ok"][b, :r["idx"][b]] if r["ret"][b] else r["ok"][b]
        assert r["cmp_new_cost"][b] == tried[-1] and r["cmp_dexp"][b] == tried.any()
        assert np.isnan(r["new_cost"][b]) == (not r["cmp_new_cost"][b]) and np.isnan(r["dcost"][b]) == np.isnan(r["expected"][b]) == (not r["cmp_dexp"][b])
    # the trajectory left behind: the accepted roll-out, else the nominal untouched
    rej = r["ret"] == 0
    assert same(r["xc"][rej], r["xn"][rej]) and same(r["uc"][rej], r["un"][rej])
    assert all(not same(r["uc"][b], r["un"][b]) for b in np.flatnonzero(~rej))


# ---------------------------------------------------------------------------
# the table discriminates: the scan restated, with the mistakes a device form could make
# ---------------------------------------------------------------------------
MUTATIONS = ("ge", "no_guard", "values_of_failed", "reset_at_boundary", "best_z", "index_off_by_one")


def scan(ok, c, alpha, cost, dV0, dV1, zmin, split, mut=None):
    """line_search.c:37-75 from the roll-outs' (ok, cost): (index, accepted, new_cost, dcost, expected); dcost / expected
    start as the sentinels (the reference's are uninitialised).  split: where a second stage would start"""
    A = len(alpha)
    dcost, expected, cnew, hit, zs = LS.SENTINEL["dcost"], LS.SENTINEL["expected"], 0.0, None, {}
    for i in range(A):
        if mut == "reset_at_boundary" and i == split:
            dcost, expected = LS.SENTINEL["dcost"], LS.SENTINEL["expected"]
        cnew = c[i]
        if not ok[i] and mut != "values_of_failed":
            continue
        dcost = cost - cnew
        expected = -alpha[i] * (dV0 + alpha[i] * dV1)
        if not ok[i]:
            continue
        z = dcost / expected if (expected > 0 or (mut == "no_guard" and expected != 0)) else 0.0
        if z >= zmin if mut == "ge" else z > zmin:
            zs[i] = z
            if mut != "best_z":
                hit = i
                break
    if mut == "best_z" and zs:
        hit = max(zs, key=zs.get)
        cnew, dcost, expected = c[hit], cost - c[hit], -alpha[hit] * (dV0 + alpha[hit] * dV1)
    none = A if mut == "index_off_by_one" else A + 1
    return (hit + 1 if hit is not None else none), int(hit is not None), cnew, dcost, expected


def outcomes(name, split, mut):
    r = LS.reference(name)
    alpha, zmin = LS.BATCHES[name][2], LS.BATCHES[name][3]
    partial = np.where(r["ok"] == 1, r["ac"], 0.25)  # (a failed roll-out's cost: any number, it is compared nowhere)
    return [scan(r["ok"][b], partial[b], alpha, r["cost"][b], r["dV0"][b], r["dV1"][b], zmin, split, mut) for b in range(len(r["cls"]))]


@pytest.mark.parametrize("name", NAMES)
def test_restated_scan_equals_the_reference(oracle_built, name):
    r = LS.reference(name)
    for b, (idx, ret, cnew, dcost, expected) in enumerate(outcomes(name, 4, None)):
        assert idx == r["idx"][b] and ret == r["ret"][b], (name, b)
        if r["cmp_new_cost"][b]:
            assert cnew == r["new_cost"][b]
        if r["cmp_dexp"][b]:
            assert dcost == r["dcost"][b] and expected == r["expected"][b]
        else:
            assert (dcost, expected) == (LS.SENTINEL["dcost"], LS.SENTINEL["expected"])


@pytest.mark.parametrize("mut", MUTATIONS)
def test_every_mistake_is_caught_by_some_case(oracle_built, mut):
    """index, acceptance or a compared left-behind value changes on at least one case (the stage boundary at the splits
    the GPU tests use)"""
    caught = []
    for name in NAMES:
        r = LS.reference(name)
        A = len(LS.BATCHES[name][2])
        for split in sorted(set(s for s in (1, 3, 4) if s < A) or {A}):
            good, bad = outcomes(name, split, None), outcomes(name, split, mut)
            for b, (g, m) in enumerate(zip(good, bad)):
                differs = g[:2] != m[:2] or (r["cmp_new_cost"][b] and g[2] != m[2]) or g[3:] != m[3:]
                if differs:
                    caught.append((name, split, b, r["cls"][b]))
    print("%s: caught by %d (batch, split, case), classes %s" % (mut, len(caught), sorted(set(c[3] for c in caught))))
    assert caught, mut
