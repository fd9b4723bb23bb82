"""The box-QP case generator of tests/boxqp_cases.py, pinned to the reference's own boxQP (oracle/_ref, FMA-free; no GPU):
the families reach every exit of boxQP.c often enough at every size the device forms are tested at, and the `mixed`
order puts unlike problems into the four rows of a wavefront.  (The reference prints H on its exit -2.)"""
import numpy as np
import pytest

from boxqp_cases import APART, OUT_OF_RANGE, SEED, cases, packings, reference

CODES = (-2, -1, 1, 2, 4, 5, 6)


@pytest.fixture(scope="module")
def ref(oracle_built):
    return {n: reference(n) for n in (1, 2, 3, 8)}


def wavefronts(order):
    return [order[i:i + 4] for i in range(0, len(order), 4)]


def test_generator_is_deterministic_and_complete():
    for n in (1, 2, 3, 8):
        a, b = cases(n), cases(n, SEED[n])
        for k in ("H", "g", "lo", "hi", "x0"):
            assert np.array_equal(a[k], b[k])
        fam = a["family"].tolist()
        want = dict(rand=240, well=120, indef=40, allclamp=40, degenerate=40, zero=20, singular=40)
        want.update({"scale-260": 30, "scale-150": 30, "scale+150": 30, "scale+260": 30})
        for k, v in want.items():
            assert fam.count(k) == v, (n, k)
        assert (fam.count("golden") > 5) == (n in (2, 8))
        assert np.all(a["lo"] <= a["hi"]) and a["H"].shape == (len(fam), n * (n + 1) // 2)
        deg = a["family"] == "degenerate"
        assert np.all((a["lo"][deg] == a["hi"][deg]).sum(axis=1) == 1)
        assert np.all(np.any((a["x0"][deg] < a["lo"][deg]) | (a["x0"][deg] > a["hi"][deg]), axis=1))  # (lo == hi: a point)


def test_every_exit_of_the_reference_is_reached(ref):
    for n in (1, 2, 3, 8):
        c, r = ref[n]
        own = c["family"] != "golden"
        count = {k: int(np.sum(r["rc"][own] == k)) for k in CODES}
        print("n = %d:" % n, count)
        if n == 1:
            assert all(count[k] >= 20 for k in (-1, 5, 6)), count
            continue
        assert all(count[k] >= 2 for k in (-2, -1, 2, 4, 5, 6)), (n, count)
        if n == 8:
            assert count[1] >= 1, count


def test_sorted_alone_and_tail_orders(ref):
    for n in (1, 2, 3, 8):
        c, r = ref[n]
        P = len(r["rc"])
        p = packings(r["rc"], P, c["family"])
        assert np.array_equal(np.sort(p["sorted"]), np.arange(P)) and np.all(np.diff(r["rc"][p["sorted"]]) >= 0)
        assert np.array_equal(np.unique(p["mixed"]), np.arange(P)) and len(p["mixed"]) % 4 == 0  # every problem, whole wavefronts
        a = p["alone"]
        assert len(a["index"]) == 4 * P and a["active"].sum() == P
        for w in (0, 1, 2, 3, P - 1):
            row = a["active"][4 * w:4 * w + 4]
            assert row.tolist() == [int(s == w % 4) for s in range(4)] and a["index"][4 * w + w % 4] == w
        assert np.all(c["family"][a["index"][a["active"] == 0]] == "indef")
        assert sorted(p["tail"]) == [1, 2, 3, 5]
        for k, v in p["tail"].items():
            assert k % 4 != 0 and np.array_equal(v, p["sorted"][:k])


def test_mixed_puts_the_out_of_range_problems_beside_plain_ones(ref):
    """every scale+-260 problem (pivots outside the short forms' range: the wavefront factorises once more in the general
    form) has at least two in-range neighbours; as the order is built, it and every indef problem (a failed factorisation)
    is the only one of its kind in its wavefront"""
    for n in (1, 2, 3, 8):
        c, r = ref[n]
        fam = c["family"]
        rows = wavefronts(packings(r["rc"], len(fam), fam)["mixed"])
        seen = 0
        for w in rows:
            out = [i for i in w if fam[i] in OUT_OF_RANGE]
            seen += len(out)
            if out:
                assert sum(fam[i] not in OUT_OF_RANGE for i in w) >= 2, (n, w)
            assert sum(fam[i] in APART for i in w) <= 1, (n, w)
            if any(fam[i] in APART for i in w):
                assert len(w) == 4
        assert seen == 60
        # the row of such a problem moves through all four positions (the shift of the row's bits in a ballot)
        at = {s for w in rows for s, i in enumerate(w) if fam[i] in APART}
        assert at == {0, 1, 2, 3}


def test_mixed_wavefronts_hold_three_or_more_codes(ref):
    """at least 90 % of the wavefronts of `mixed` hold three or more different reference codes.  (A wavefront with three
    codes holds at least two problems whose code is not the commonest one, and three quarters of the problems end with 5:
    an order that takes every problem ONCE cannot reach half of that — which is why `mixed` hands the problems of rare
    codes out again.  Obtained: every wavefront, with 812 to 1 036 rows for 660 to 685 problems.)"""
    for n in (1, 2, 3, 8):
        c, r = ref[n]
        order = packings(r["rc"], len(r["rc"]), c["family"])["mixed"]
        rows = wavefronts(order)
        three = sum(len(set(r["rc"][w].tolist())) >= 3 for w in rows)
        print("n = %d: %d rows for %d problems, %d wavefronts, %d with three or more codes, a problem at most %d times"
              % (n, len(order), len(r["rc"]), len(rows), three, np.bincount(order).max()))
        assert three >= 0.9 * len(rows), (n, three, len(rows))
