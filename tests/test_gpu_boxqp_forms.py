"""The four device restatements of boxQP.c (ilqg_rules.h) directly against the reference's own boxQP and against each other,
on the problems of tests/boxqp_cases.py (every exit of the reference at every size; tests/test_boxqp_cases_recipe.py):

    box_qp<M>        one problem per lane               boxqp_batch(n, ...)                     M = 1, 2, 3, 8
    box_qp_row<M>    one problem per wavefront          boxqp_batch(n, ..., cooperative=True)   M = 3 (2, 8: test_gpu_parity.py)
    box_qp_rows<M>   the same, one element per lane     ... of the `_elem` library               M = 2, 8
    box_qp_quad<M>   four problems per wavefront        boxqp_batch(n, ..., cooperative="quad") M = 2, 8

FMA-free builds: the reference's bits.  Product builds (FMA contraction): the reference's exit and clamp flags and its
solution to 1e-12 on the families whose exits are not taken at rounding resolution (boxqp_cases.PRODUCT_FAMILIES), the
product rule of test_boxqp_golden on the goldens.  box_qp_quad shares one instruction stream among four unrelated
problems: what a row computes must not depend on its neighbours, in any build."""
import numpy as np
import pytest

from boxqp_cases import PRODUCT_FAMILIES, check_product_golden, packings, reference
from conftest import golden

pytestmark = pytest.mark.gpu

SYN = dict(problem="synth16x8", full_ddp=1)
OUT = ("rc", "clamp", "n_free", "x", "invH")


@pytest.fixture(scope="module")
def ilqg():
    import __graft_entry__ as g
    g.build_for_tests()
    from ddp_generator_amd import ilqg as m
    if m.Problem("carparking", 0).device_count() < 1:
        pytest.fail("no HIP device visible: the GPU tests must run on the MI355X box")
    return m


def same(a, b):
    return np.array_equal(a, b, equal_nan=True)


def differing(a, b):
    """indices of the problems whose rows of a and b differ in some bit"""
    a, b = a.reshape(len(a), -1), b.reshape(len(b), -1)
    return np.nonzero(~np.all((a == b) | ((a != a) & (b != b)), axis=1))[0]


def solve(ilqg, n, order=None, x0=None, **kw):
    """the device form selected by kw on the problems of cases(n) in the order given (default: as generated)"""
    c, _ = reference(n)
    order = np.arange(len(c["H"])) if order is None else order
    return ilqg.boxqp_batch(n, c["H"][order], c["g"][order], c["lo"][order], c["hi"][order], c["x0"][order] if x0 is None else x0, **kw)


_quad = {}


def quad(ilqg, n, build):
    """box_qp_quad<n> of the synth16x8 library `build` in the orders sorted / mixed / alone: {packing: {output: [...]}} with
    sorted and alone brought back to the generator's order, mixed as run (row s holds problem mixed_order[s]), and the raw
    results of `alone` (all 4 P rows)"""
    if (n, build) in _quad:
        return _quad[n, build]
    c, r = reference(n)
    P = len(r["rc"])
    p = packings(r["rc"], P, c["family"])
    out = {}
    got = solve(ilqg, n, p["sorted"], strict=build, cooperative="quad", **SYN)
    inv = np.argsort(p["sorted"])
    out["sorted"] = {k: got[k][inv] for k in OUT}
    got = solve(ilqg, n, p["mixed"], strict=build, cooperative="quad", **SYN)
    out["mixed"] = {k: got[k] for k in OUT}  # (row by row: `mixed` holds the problems of rare codes more than once)
    out["mixed_order"] = p["mixed"]
    a = p["alone"]
    x0 = c["x0"][a["index"]].copy()
    x0[a["active"] == 0] += 7.0  # the rows that are not active start outside their box
    assert np.all(np.any(x0[a["active"] == 0] > c["hi"][a["index"]][a["active"] == 0], axis=1))
    got = solve(ilqg, n, a["index"], x0=x0, strict=build, cooperative="quad", active=a["active"], **SYN)
    out["alone"] = {k: got[k][a["slot"]] for k in OUT}
    out["alone_raw"] = dict(got, x0=x0)
    _quad[n, build] = out
    return out


def check_bits_of_reference(got, ref, what):
    for k in ("rc", "clamp", "n_free", "x"):
        d = differing(np.asarray(got[k]), ref[k])
        assert len(d) == 0, (what, k, len(d), d[:8], got["rc"][d[:8]], ref["rc"][d[:8]])


def check_bits_of_each_other(a, b, what):
    """rc, clamp, x, and the inverse where a factorisation stands behind it (rc -1: the inverse of an earlier one, or zeros)"""
    for k in ("rc", "clamp", "x"):
        d = differing(a[k], b[k])
        assert len(d) == 0, (what, k, len(d), d[:8])
    ok = a["rc"] != -1
    d = differing(a["invH"][ok], b["invH"][ok])
    assert len(d) == 0, (what, "invH", len(d), np.nonzero(ok)[0][d[:8]])


def check_product_rule(got, n, what):
    """the product build against the reference: exit, clamp flags and x to 1e-12 on PRODUCT_FAMILIES (nothing left out),
    the goldens by the product branch of test_boxqp_golden"""
    c, ref = reference(n)
    sel = np.nonzero(np.isin(c["family"], PRODUCT_FAMILIES))[0]
    assert len(sel) == 260
    bad = [i for i in sel if got["rc"][i] != ref["rc"][i] or not np.array_equal(got["clamp"][i], ref["clamp"][i])]
    assert not bad, (what, [(i, c["family"][i], int(got["rc"][i]), int(ref["rc"][i])) for i in bad[:8]])
    err = np.abs(got["x"][sel] - ref["x"][sel]) / np.maximum(1.0, np.abs(ref["x"][sel]))
    print("%s: worst deviation of x from the reference %.3g" % (what, err.max()))
    assert err.max() <= 1e-12, (what, err.max(), c["family"][sel[np.argmax(err.max(axis=1))]])
    g = golden("kernels.npz")
    for i in np.nonzero(c["golden"] >= 0)[0]:
        check_product_golden(int(got["rc"][i]), got["x"][i], got["clamp"][i], int(got["n_free"][i]), g, int(c["golden"][i]), n)


# ---------------------------------------------------------------------------
# a. box_qp_quad does not depend on its neighbours
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("n", [8, 2])
@pytest.mark.parametrize("build", [False, True, "lean"])
def test_quad_rows_do_not_depend_on_their_neighbours(ilqg, n, build):
    """every problem gives the same bits whether its wavefront holds problems of its own exit code (sorted), of other
    codes, ranges and definiteness (mixed: three or more codes in every wavefront, problems of rare codes beside several
    sets of neighbours), or nothing else (alone: three rows not active) — in the product build too:
    it is one instruction stream per build, and the short forms of sqrt / reciprocal / quotient give the general forms'
    bits in their range (tests/test_short_quotient.py)"""
    q = quad(ilqg, n, build)
    c, r = reference(n)
    for other, order in (("mixed", q["mixed_order"]), ("alone", np.arange(len(r["rc"])))):
        for k in ("rc", "clamp", "x"):
            d = np.unique(order[differing(q["sorted"][k][order], q[other][k])])
            print("n = %d, build %r: %d problems differ in %s between sorted and %s" % (n, build, len(d), k, other))
            assert len(d) == 0, (other, k, len(d), d[:8], c["family"][d[:8]], r["rc"][d[:8]])
        ok = q["sorted"]["rc"][order] != -1
        d = differing(q["sorted"]["invH"][order][ok], q[other]["invH"][ok])
        assert len(d) == 0, (other, "invH", len(d), order[ok][d[:8]])
    assert same(q["sorted"]["n_free"], n - (q["sorted"]["clamp"] != 0).sum(axis=1))
    assert len(set(q["sorted"]["rc"].tolist())) >= 5


@pytest.mark.parametrize("n", [8, 2])
@pytest.mark.parametrize("build", [False, True, "lean"])
def test_quad_tail_wavefronts_and_inactive_rows(ilqg, n, build):
    """a last wavefront with one, two or three problems (rows beyond the count load and store nothing) gives the first
    results of the full order; a row that is not active keeps its x bit for bit — outside its box too —, returns 0 and
    leaves the result of the one active row of its wavefront what it is in a full wavefront"""
    q = quad(ilqg, n, build)
    c, r = reference(n)
    p = packings(r["rc"], len(r["rc"]), c["family"])
    for count, order in sorted(p["tail"].items()):
        got = solve(ilqg, n, order, strict=build, cooperative="quad", **SYN)
        for k in OUT:
            assert same(got[k], q["sorted"][k][order]), (count, k)
    raw, a = q["alone_raw"], p["alone"]
    off = a["active"] == 0
    assert same(raw["x"][off], raw["x0"][off]) and np.all(raw["rc"][off] == 0)
    assert np.all(raw["rc"][~off] != 0)
    for k in ("rc", "clamp", "x"):
        assert same(raw[k][a["slot"]], q["sorted"][k])
    # active = None is every row active
    one = solve(ilqg, n, p["mixed"][:12], strict=build, cooperative="quad", active=np.ones(12, dtype=np.int32), **SYN)
    for k in OUT:
        assert same(one[k], q["mixed"][k][:12]), k


@pytest.mark.parametrize("n", [8, 2])
def test_quad_lean_layout_equals_the_default_on_every_problem(ilqg, n):
    """the factor's diagonal in LDS instead of registers (ilqg_quad.hpp ILQG_QUAD_LEAN) changes no bit of any output"""
    a, b = quad(ilqg, n, False), quad(ilqg, n, "lean")
    for name in ("sorted", "mixed", "alone"):
        for k in OUT:
            d = differing(a[name][k], b[name][k])
            assert len(d) == 0, (name, k, len(d), d[:8])


# ---------------------------------------------------------------------------
# b. box_qp_quad against the reference and the per-lane form
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("n", [8, 2])
def test_quad_gives_the_reference_bits_in_the_fma_free_build(ilqg, n):
    q = quad(ilqg, n, True)["sorted"]
    _, ref = reference(n)
    check_bits_of_reference(q, ref, "box_qp_quad<%d>" % n)
    lane = solve(ilqg, n, strict=True, **SYN)
    check_bits_of_each_other(q, lane, "box_qp_quad<%d> against box_qp<%d>" % (n, n))


@pytest.mark.parametrize("n", [8, 2])
def test_quad_product_build_against_the_reference(ilqg, n):
    check_product_rule(quad(ilqg, n, False)["sorted"], n, "box_qp_quad<%d>" % n)


# ---------------------------------------------------------------------------
# c. box_qp_rows (the `_elem` library: the one-output-element-per-lane step, FMA-free)
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("n", [8, 2])
def test_rows_form_gives_the_reference_bits(ilqg, n):
    rows = solve(ilqg, n, strict="elem", cooperative=True, **SYN)
    _, ref = reference(n)
    check_bits_of_reference(rows, ref, "box_qp_rows<%d>" % n)
    lane = solve(ilqg, n, strict=True, **SYN)
    check_bits_of_each_other(rows, lane, "box_qp_rows<%d> against box_qp<%d>" % (n, n))
    assert same(rows["n_free"], lane["n_free"])


# ---------------------------------------------------------------------------
# d. the odd sizes: N_U = 1 (brachi) and N_U = 3 (synth10hx; its backward pass runs box_qp_row<3>)
# ---------------------------------------------------------------------------
ODD = {1: dict(problem="brachi", full_ddp=0), 3: dict(problem="synth10hx", full_ddp=1)}


@pytest.mark.parametrize("n", [1, 3])
def test_odd_sizes_give_the_reference_bits_in_the_fma_free_build(ilqg, n):
    _, ref = reference(n)
    lane = solve(ilqg, n, strict=True, **ODD[n])
    check_bits_of_reference(lane, ref, "box_qp<%d>" % n)
    if n == 3:
        row = solve(ilqg, n, strict=True, cooperative=True, **ODD[n])
        check_bits_of_reference(row, ref, "box_qp_row<3>")
        check_bits_of_each_other(row, lane, "box_qp_row<3> against box_qp<3>")


@pytest.mark.parametrize("n", [1, 3])
def test_odd_sizes_product_build_against_the_reference(ilqg, n):
    check_product_rule(solve(ilqg, n, **ODD[n]), n, "box_qp<%d>" % n)
    if n == 3:
        check_product_rule(solve(ilqg, n, cooperative=True, **ODD[n]), n, "box_qp_row<3>")


@pytest.mark.parametrize("strict", [False, True])
def test_one_variable_by_hand(ilqg, strict):
    """n = 1 needs no reference: where the solver ends regularly (5, 6) on a convex problem, x is clip(-g / H, lo, hi) to
    1e-12 relative.  One exception follows from boxQP.c's gradient exit being ABSOLUTE (|g + H x| < 1e-8, which the
    problems scaled by 2^-150 and 2^-260 meet wherever they start; the reference does the same): a problem whose gradient
    at the clipped warm start is that small leaves at once with 5 and keeps the clipped warm start, bit for bit."""
    c, _ = reference(1)
    got = solve(ilqg, 1, strict=strict, **ODD[1])
    H, g, lo, hi, x0 = (c[k][:, 0] for k in ("H", "g", "lo", "hi", "x0"))
    start = np.clip(x0, lo, hi)
    grad = g + H * start
    at_limit = ((start <= lo) & (grad > 0)) | ((start >= hi) & (grad < 0))
    at_once = ~at_limit & (grad * grad < 1e-8 * 1e-8)
    regular = np.isin(got["rc"], (5, 6)) & (H > 0)
    assert regular.sum() > 500 and (regular & at_once).sum() > 20 and (regular & ~at_once).sum() > 400
    x = got["x"][:, 0]
    assert np.all(got["rc"][regular & at_once] == 5) and same(x[regular & at_once], start[regular & at_once])
    s = regular & ~at_once
    want = np.clip(-g[s] / H[s], lo[s], hi[s])
    err = np.abs(x[s] - want)
    print("worst relative deviation from clip(-g / H, lo, hi): %.3g" % np.max(err / np.maximum(np.abs(want), 1e-300)))
    assert np.all(err <= 1e-12 * np.abs(want))
