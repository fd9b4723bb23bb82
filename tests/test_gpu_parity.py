"""GPU parity tests: the HIP path (through the C-ABI) against the CPU oracle and
against the golden fixtures recorded from the reference.

Tolerances (BASELINE.json north_star "within a stated fp64
tolerance"): single-pass quantities |d| <= 1e-10 * max(1, |ref|) elementwise;
return codes, clamp flags and accepted step-size indices must be EQUAL; full
solves: final cost rel 1e-6, trajectory abs 1e-4.  The device code differs from
the CPU only by fused multiply-add contraction and the device math library.
"""
import numpy as np
import pytest

from boxqp_cases import check_product_golden
from conftest import golden, load_package
from oracle.harness import CAR_PARAMS, HX_N, HX_PARAMS, SYN_PARAMS, SYN_PARAMS_TIGHT, SYNP_PARAMS_TIGHT, Driver, hx_inputs, lib_path, syn_inputs

SYN_TIGHT = SYN_PARAMS_TIGHT

pytestmark = pytest.mark.gpu

TOL = 1e-10


def close(a, b, tol=TOL):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return bool(np.all(np.abs(a - b) <= tol * np.maximum(1.0, np.abs(b))))


def worst(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.max(np.abs(a - b) / np.maximum(1.0, np.abs(b))))


@pytest.fixture(scope="module")
def ilqg():
    import __graft_entry__ as g
    g.build_for_tests()  # (with the `_strict`, `_exp`, `_lean`, `_elem` libraries tests of this module load)
    from ddp_generator_amd import ilqg as m
    if m.Problem("carparking", 0).device_count() < 1:
        pytest.fail("no HIP device visible: the GPU tests must run on the MI355X box")
    return m


@pytest.fixture(scope="module")
def synth():
    return load_package().synth


def tri(n):
    return n * (n + 1) // 2


# ---------------------------------------------------------------------------
# unit: device box-QP against the reference's golden vectors (every reachable rc)
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("n", [2, 8])
@pytest.mark.parametrize("strict", [False, True])
def test_boxqp_golden(ilqg, n, strict):
    """strict (-ffp-contract=off) build: EXACT agreement on every golden, including the
    rounding-chaotic ones.  Product build (FMA contraction): return code 2 (Armijo step below
    1e-22, boxQP.c:222-224) is only reached when the objective change is below rounding
    resolution, so whether such a problem ends as 2 or 4 depends on the last bit; those
    goldens are checked on the strict build only."""
    g = golden("kernels.npz")
    sel = np.nonzero(g["qp_n"] == n)[0]
    assert len(sel) > 5
    t = tri(n)
    r = ilqg.boxqp_batch(n, g["qp_H"][sel][:, :t], g["qp_g"][sel][:, :n], g["qp_lo"][sel][:, :n],
                         g["qp_hi"][sel][:, :n], g["qp_x0"][sel][:, :n], strict=strict)
    for j, i in enumerate(sel):
        rc = int(g["qp_rc"][i])
        if strict:
            assert r["rc"][j] == rc
            assert np.array_equal(r["clamp"][j], g["qp_clamp"][i][:n]) and r["n_free"][j] == g["qp_nfree"][i]
            assert np.array_equal(r["x"][j], g["qp_x"][i][:n]), (i, rc)
            continue
        # product build: the exits taken at rounding resolution may differ (boxqp_cases.check_product_golden states the rule,
        # also for the quad form's test in test_gpu_boxqp_forms.py)
        check_product_golden(int(r["rc"][j]), r["x"][j], r["clamp"][j], int(r["n_free"][j]), g, i, n)


@pytest.mark.parametrize("n", [2, 8])
@pytest.mark.parametrize("strict", [False, True])
def test_cooperative_boxqp_equals_the_per_lane_one(ilqg, n, strict):
    """box_qp_row (wave mapping: one lane per variable, operands broadcast) computes every scalar by the same
    expression tree as the per-lane template: identical results bit for bit in the -ffp-contract=off build, on the
    reference's goldens (every exit) and on random problems"""
    g = golden("kernels.npz")
    sel = np.nonzero(g["qp_n"] == n)[0]
    t = tri(n)
    rng = np.random.default_rng(3 + n)
    R = 400
    A = rng.standard_normal((R, n, n))
    Mx = A @ np.transpose(A, (0, 2, 1)) + (10.0 ** rng.uniform(-8, 0, R))[:, None, None] * np.eye(n)
    H = np.concatenate([g["qp_H"][sel][:, :t], np.array([[m[r, c] for c in range(n) for r in range(c + 1)] for m in Mx])])
    gg = np.concatenate([g["qp_g"][sel][:, :n], rng.standard_normal((R, n))])
    lo = np.concatenate([g["qp_lo"][sel][:, :n], -np.abs(rng.standard_normal((R, n)))])
    hi = np.concatenate([g["qp_hi"][sel][:, :n], np.abs(rng.standard_normal((R, n)))])
    x0 = np.concatenate([g["qp_x0"][sel][:, :n], rng.standard_normal((R, n))])
    # the cooperative form takes short forms of sqrt / reciprocal / quotient while the pivots lie in [2^-200, 2^200] and
    # the compiler's general ones otherwise: the last 120 random problems are scaled so that both happen with large and
    # with small numbers (pivots ~ 2^+-150: short forms; ~ 2^+-260: general)
    scale = np.ones(len(H))
    scale[-120:] = np.repeat(2.0 ** np.array([-260.0, -150.0, 150.0, 260.0]), 30)
    H = H * scale[:, None]
    gg = gg * scale[:, None]
    a = ilqg.boxqp_batch(n, H, gg, lo, hi, x0, strict=strict)
    b = ilqg.boxqp_batch(n, H, gg, lo, hi, x0, strict=strict, cooperative=True)
    assert len(set(a["rc"].tolist())) >= 4
    if strict:
        assert np.array_equal(a["rc"], b["rc"]) and np.array_equal(a["n_free"], b["n_free"])
        assert np.array_equal(a["clamp"], b["clamp"])
        assert np.array_equal(a["x"], b["x"], equal_nan=True)
        ok = a["rc"] != -1  # a failed factorisation leaves the inverse of the previous one (or zeros) in both
        assert np.array_equal(a["invH"][ok], b["invH"][ok], equal_nan=True)
        return
    # product build: the compiler contracts the two code shapes into FMAs differently, so values agree to rounding
    # and an exit taken at rounding resolution (see test_boxqp_golden) may differ
    same = (a["rc"] == b["rc"]) & np.all(a["clamp"] == b["clamp"], axis=1)
    assert same[scale == 1.0].mean() > 0.97, same[scale == 1.0].mean()
    # (the scaled problems meet the absolute thresholds of boxQP.c — gradient 1e-8, improvement 1e-8 relative — at
    # rounding resolution far more often; bit-equality on them is what the strict build asserts above)
    assert same[scale != 1.0].mean() > 0.7, same[scale != 1.0].mean()
    reg = same & (a["rc"] >= 2)  # (rc 1: 100 iterations on a numerically singular Hessian, rounding-chaotic)
    scale = np.maximum(1.0, np.abs(a["x"][reg]).max(axis=1, keepdims=True))
    assert np.all(np.abs(a["x"][reg] - b["x"][reg]) <= 1e-7 * scale)


@pytest.mark.parametrize("strict", [False, True])
def test_boxqp_with_pattern_table_equals_the_in_loop_factorisation(ilqg, strict):
    """box_qp<2, TABLE> (factor and inverse of the free block for all three clamp patterns before the iteration, selected
    by pattern inside it; ilqg_device.hpp chol_pattern_table) against the form that factorises when the free set changes:
    the same bits in every output, every exit, in both builds — goldens, random problems, problems scaled out of the
    short forms' range"""
    n, t = 2, 3
    g = golden("kernels.npz")
    sel = np.nonzero(g["qp_n"] == n)[0]
    rng = np.random.default_rng(11)
    R = 600
    A = rng.standard_normal((R, n, n))
    Mx = A @ np.transpose(A, (0, 2, 1)) + (10.0 ** rng.uniform(-8, 0, R))[:, None, None] * np.eye(n)
    Mx[:40] -= 2.0 * np.eye(n)  # indefinite ones: failed factorisations (rc -1) of the visited pattern only
    H = np.concatenate([g["qp_H"][sel][:, :t], np.array([[m[r, c] for c in range(n) for r in range(c + 1)] for m in Mx])])
    gg = np.concatenate([g["qp_g"][sel][:, :n], rng.standard_normal((R, n))])
    lo = np.concatenate([g["qp_lo"][sel][:, :n], -np.abs(rng.standard_normal((R, n)))])
    hi = np.concatenate([g["qp_hi"][sel][:, :n], np.abs(rng.standard_normal((R, n)))])
    x0 = np.concatenate([g["qp_x0"][sel][:, :n], rng.standard_normal((R, n))])
    scale = np.ones(len(H))
    scale[-120:] = np.repeat(2.0 ** np.array([-260.0, -150.0, 150.0, 260.0]), 30)
    H, gg = H * scale[:, None], gg * scale[:, None]
    exp = "exp_strict" if strict else "exp"  # (the pattern tables are compiled into the -DILQG_EXPERIMENTS libraries only)
    a = ilqg.boxqp_batch(n, H, gg, lo, hi, x0, strict=exp)
    b = ilqg.boxqp_batch(n, H, gg, lo, hi, x0, strict=exp, cooperative="table")
    assert len(set(a["rc"].tolist())) >= 5 and (a["rc"] == -1).sum() > 3 and (a["n_free"] == 1).sum() > 20
    for k in ("rc", "n_free", "clamp"):
        assert np.array_equal(a[k], b[k]), k
    assert np.array_equal(a["x"], b["x"], equal_nan=True) and np.array_equal(a["invH"], b["invH"], equal_nan=True)


def test_search_without_memory_for_the_kept_rollouts_falls_back(ilqg, synth, monkeypatch):
    """ls_keep = 2 wants two sets of planes of the size of X / U; a device that cannot provide them searches in the
    ls_keep = 1 form instead of failing — same results (FMA-free build: the same bits)"""
    B, N, K = 200, 500, 6
    x0, u0 = synth.car_batch(B, N)

    def run():
        s = ilqg.BatchSolver("carparking", 0, batch=B, n_hor=N, params=ilqg.CAR_PARAMS, opts=dict(max_iter=K), strict=True)
        s.init(x0, u0)
        s.iterate(K)
        out = (s.scalar("cost").copy(), s.x().copy(), s.u().copy(), s.ints("alpha_idx").copy())
        s.close()
        return out

    a = run()
    monkeypatch.setenv("ILQG_TEST_NO_PLANES", "1")
    b = run()
    for p, q in zip(a, b):
        assert np.array_equal(p, q)


def test_device_sincos_accuracy(ilqg):
    """the straight-line sincos the callbacks' sin()/cos() are routed through: within 2 ulp of the host
    libm below 8e5 (small, medium, large arguments and next to multiples of pi/2); beyond that, for NaN
    and Inf it defers to the device library — checked against exact (mpmath) values there, because the
    host's vectorised libm is itself not trustworthy for huge arguments"""
    import mpmath
    rng = np.random.default_rng(5)
    parts = [rng.uniform(-s, s, 50000) for s in (1e-3, 1.0, 10.0, 1e3, 7.9e5)]
    k = rng.integers(-500000, 500000, 50000)
    parts.append(k * (np.pi / 2) * (1 + rng.uniform(-4, 4, 50000) * 2.2e-16))
    parts.append(np.array([0.0, -0.0, np.pi, np.pi / 2, 355.0, 7.99e5, -7.99e5]))
    x = np.concatenate(parts)
    s, c = ilqg.sincos_batch(x)
    for got, want in ((s, np.sin(x)), (c, np.cos(x))):
        ulp = np.abs(got - want) / np.spacing(np.abs(want))
        assert ulp.max() <= 2.0, ulp.max()
        assert np.mean(ulp > 0) < 0.35
    # huge arguments: library fallback, exact reference
    mpmath.mp.prec = 1200
    xh = np.concatenate([rng.uniform(-1, 1, 150) * 10.0 ** rng.uniform(6, 300, 150), [8.0e5, -8.0e5, 1e12, 1e300]])
    s, c = ilqg.sincos_batch(xh)
    for i, xv in enumerate(xh):
        es, ec = float(mpmath.sin(mpmath.mpf(float(xv)))), float(mpmath.cos(mpmath.mpf(float(xv))))
        assert abs(s[i] - es) <= 2 * np.spacing(abs(es)) and abs(c[i] - ec) <= 2 * np.spacing(abs(ec)), (xv, s[i], es)
    s, c = ilqg.sincos_batch(np.array([np.nan, np.inf, -np.inf]))
    assert np.all(np.isnan(s)) and np.all(np.isnan(c))


def test_dropin_dense_helpers_golden(ilqg):
    """the reference's matMult / Cholesky symbols exported by the product library run the device templates"""
    import os
    from conftest import ROOT
    from oracle.harness import Kernels
    g = golden("kernels.npz")
    K = Kernels(ilqg.library_path("carparking", 0))
    p = lambda k: g["mm_car_" + k]
    assert close(K.add_mul_vec(p("base_u"), p("vx"), p("fu"), 4, 2), p("mulvec"), 1e-13)
    assert close(K.add_square_tri(p("base_uu"), p("V"), p("fu"), 4, 2), p("sq_uu"), 1e-13)
    assert close(K.add_square_tri(p("base_xx"), p("V"), p("fx"), 4, 4), p("sq_xx"), 1e-13)
    assert close(K.add_mul2_tri(p("base_xu"), p("V"), p("fx"), 4, 4, p("fu"), 4, 2), p("mul2"), 1e-13)
    for n, A, ok, U, inv in zip(g["chol_n"], g["chol_A"], g["chol_ok"], g["chol_U"], g["chol_inv"]):
        t = tri(int(n))
        ok2, U2 = K.cholesky(A[:t].copy(), int(n))
        assert ok2 == ok
        if ok:
            assert close(U2, U[:t], 1e-13)
            assert close(K.cholesky_inv(U[:t].copy(), int(n)), inv[:t], 1e-11)
    # boxQP through the reference's own signature (free-block numbering of invHfree)
    sel = np.nonzero((g["qp_n"] == 2) & (g["qp_rc"] == 5))[0][:3]
    for i in sel:
        r = K.boxqp(g["qp_H"][i][:3], g["qp_g"][i][:2], g["qp_lo"][i][:2], g["qp_hi"][i][:2], g["qp_x0"][i][:2])
        assert r["rc"] == 5 and np.array_equal(r["clamp"], g["qp_clamp"][i][:2])
        nf = r["n_free"]
        scale = max(1.0, np.abs(g["qp_invH"][i][:tri(nf)]).max())
        assert np.all(np.abs(r["invH"][:tri(nf)] - g["qp_invH"][i][:tri(nf)]) <= 1e-9 * scale)


def test_boxqp_random_vs_oracle(ilqg, oracle_built):
    from oracle.harness import Kernels
    K = Kernels(lib_path("oracle"))
    rng = np.random.default_rng(11)
    n, count = 2, 512
    H = np.zeros((count, 3)); g = rng.standard_normal((count, n))
    lo = -np.abs(rng.standard_normal((count, n))); hi = np.abs(rng.standard_normal((count, n)))
    x0 = rng.standard_normal((count, n))
    for i in range(count):
        A = rng.standard_normal((n, n)); M = A @ A.T + 1e-3 * np.eye(n)
        H[i] = [M[0, 0], M[0, 1], M[1, 1]]
    r = ilqg.boxqp_batch(n, H, g, lo, hi, x0)
    for i in range(count):
        o = K.boxqp(H[i], g[i], lo[i], hi[i], x0[i])
        assert r["rc"][i] == o["rc"] and np.array_equal(r["clamp"][i], o["clamp"])
        assert close(r["x"][i], o["x"], 1e-12)


# ---------------------------------------------------------------------------
# single backward pass + line search on the reference demo problem (goldens)
# ---------------------------------------------------------------------------
# variant "_plain": the same problem emitted without any additive hint or table (tools/gen_problem.py --plain, what a
# Maxima/gentran-generated pair looks like): the kernels' general-case branches (state-dependent limits assumed, every
# record entry treated as time varying, stored tensors)
@pytest.mark.parametrize("variant", ["", "_plain"])
@pytest.mark.parametrize("fd", [0, 1])
def test_single_pass_golden(ilqg, fd, variant):
    check_single_pass(ilqg, "carparking" + variant, fd)


def check_single_pass(ilqg, problem, fd):
    """(also run on CarParking libraries built from other directories: tests/test_out_of_tree.py, test_template_literal.py)"""
    g = golden("car_single_fd%d.npz" % fd)
    # ls_split=0: every step size is rolled out, so all eight per-alpha costs can be compared
    s = ilqg.BatchSolver(problem, fd, batch=1, n_hor=500, params=ilqg.CAR_PARAMS, opts=dict(ls_split=0))
    s.init(g["x0"][None], g["u0"][None])
    assert close(s.scalar("cost")[0], g["init_cost"])
    assert close(s.x()[0], g["x_nom"]) and close(s.u()[0], g["u_nom"])

    s.calc_derivs()
    rec, fin = s.derivs()
    nd = s.problem.rec_dev
    assert close(rec[0][:, :nd], g["rec"][:, :nd]), worst(rec[0][:, :nd], g["rec"][:, :nd])
    assert close(fin[0], g["fin"])

    s.back_pass(single_sweep=True)
    assert s.ints("bp_rc")[0] == int(g["bp_rc"]) == 0
    l, L = s.gains()
    assert close(l[0], g["l"]), worst(l[0], g["l"])
    assert close(L[0], g["L"]), worst(L[0], g["L"])
    assert close(s.scalar("dV0")[0], g["dV"][0]) and close(s.scalar("dV1")[0], g["dV"][1])
    assert close(s.scalar("g_norm")[0], g["g_norm"])

    s.line_search()
    na = len(g["alphas"])
    assert np.array_equal(s.ints("alpha_ok")[0][:na], g["alpha_ok"])
    assert close(s.scalar("alpha_cost")[0][:na], g["alpha_cost"])
    assert s.ints("accepted")[0] == int(g["ls_accept"])
    assert s.ints("alpha_idx")[0] == int(g["ls_index"])
    assert close(s.scalar("new_cost")[0], g["new_cost"])
    assert close(s.scalar("dcost")[0], g["dcost"], 1e-9) and close(s.scalar("expected")[0], g["expected"])
    # the re-rolled winner reproduces the cost its selection was based on, bit for bit
    assert s.scalar("new_cost")[0] == s.scalar("alpha_cost")[0][int(g["ls_index"]) - 1]
    assert close(s.x()[0], g["x_cand"]) and close(s.u()[0], g["u_cand"])
    s.close()


@pytest.mark.parametrize("fd", [0, 1])
def test_backward_pass_from_golden_derivatives(ilqg, fd):
    """the kernel alone: reference derivative records in, gains out (iteration 12: clamped inputs)"""
    g = golden("car_single_fd%d.npz" % fd)
    s = ilqg.BatchSolver("carparking", fd, batch=1, n_hor=500, params=ilqg.CAR_PARAMS)
    s.init(g["x0"][None], g["u0"][None])
    for tag, lam in (("it12_", float(g["it12_lam"])),):
        # nominal u is read by the backward pass for g_norm only; put the golden one in place
        s.lib.ilqg_batch_set_u(s.h, np.ascontiguousarray(g[tag + "u"][None]))
        s.set_derivs(g[tag + "rec"][None], g[tag + "fin"][None])
        s.set_scalar("lambda", lam)
        s.back_pass(single_sweep=True)
        assert s.ints("bp_rc")[0] == int(g[tag + "rc"])
        l, L = s.gains()
        assert close(l[0], g[tag + "l"]), worst(l[0], g[tag + "l"])
        assert close(L[0], g[tag + "L"]), worst(L[0], g[tag + "L"])
        assert close(s.scalar("dV0")[0], g[tag + "dV"][0]) and close(s.scalar("dV1")[0], g[tag + "dV"][1])
        assert close(s.scalar("g_norm")[0], g[tag + "g_norm"])
    # forced Cholesky failure (back_pass.c:168-171 -> 1)
    s.set_derivs(g["bad_rec"][None], g["fin"][None])
    s.set_scalar("lambda", 1.0)
    s.back_pass(single_sweep=True)
    assert s.ints("bp_rc")[0] == int(g["bad_rc"]) == 1
    s.close()


@pytest.mark.parametrize("variant", ["", "_plain"])
@pytest.mark.parametrize("fd", [0, 1])
def test_fused_backward_matches_golden(ilqg, fd, variant):
    """derivatives evaluated inside the backward kernel: same gains as from the stored records"""
    g = golden("car_single_fd%d.npz" % fd)
    s = ilqg.BatchSolver("carparking" + variant, fd, batch=1, n_hor=500, params=ilqg.CAR_PARAMS)
    s.init(g["x0"][None], g["u0"][None])
    s.back_pass(fused=True)
    assert s.ints("bp_rc")[0] == 0 and s.ints("bp_calls")[0] == 1
    l, L = s.gains()
    assert close(l[0], g["l"]), worst(l[0], g["l"])
    assert close(L[0], g["L"]), worst(L[0], g["L"])
    assert close(s.scalar("dV0")[0], g["dV"][0]) and close(s.scalar("dV1")[0], g["dV"][1])
    assert close(s.scalar("g_norm")[0], g["g_norm"])
    s.close()


@pytest.mark.parametrize("fuse", [0, 1])
def test_fused_and_unfused_iterations_agree(ilqg, synth, fuse):
    B, iters = 70, 4
    x0, u0 = synth.car_batch(B, first=300)
    out = []
    for f in (fuse, 1 - fuse):
        s = ilqg.BatchSolver("carparking", 0, batch=B, n_hor=500, params=ilqg.CAR_PARAMS, opts=dict(max_iter=iters, fuse_derivs=f))
        s.init(x0, u0)
        s.iterate(iters)
        out.append((s.scalar("cost"), s.ints("alpha_idx"), s.x()))
        s.close()
    assert close(out[0][0], out[1][0], 1e-9) and np.array_equal(out[0][1], out[1][1])
    assert np.abs(out[0][2] - out[1][2]).max() < 1e-7


@pytest.mark.parametrize("strict", [False, True])
def test_line_search_staging_and_resweep_do_not_change_results(ilqg, synth, strict):
    """two-stage line search (any split) == all step sizes for every trajectory, bit for bit;
    the reference's cost-only re-sweep after an accepted step returns the same cost bit for bit.
    Three implementations of the stages (option ls_keep): 2 = every roll-out is kept where it is rolled out and the
    accepted one becomes the current trajectory by a change of its location index (k_search / k_commit; the lane
    mapping's default, first stages of up to 4 step sizes); 1 = second stage beside the re-rolled winners of the
    first, its own winners copied; 0 = everything accepted is rolled out again.  Within one implementation every split
    gives identical bits; ACROSS implementations (different kernels around the same generated callbacks) identical
    bits are required of the -ffp-contract=off build, the product build may contract multiply-adds differently and is
    held to the single-pass tolerance."""
    B, iters = 200, 6
    x0, u0 = synth.car_batch(B, first=900)
    ref = {}
    for opts in (dict(ls_split=4, resweep=1), dict(ls_split=3, resweep=0), dict(ls_split=1, resweep=0), dict(ls_split=2, resweep=1),
                 dict(ls_split=0, ls_keep=1), dict(ls_split=3, ls_keep=1), dict(ls_split=1, ls_keep=1), dict(ls_split=5, ls_keep=1, resweep=1),
                 dict(ls_split=8, ls_keep=1), dict(ls_split=3, ls_keep=0), dict(ls_split=2, ls_keep=0)):
        s = ilqg.BatchSolver("carparking", 0, batch=B, n_hor=500, params=ilqg.CAR_PARAMS,
                             opts=dict(max_iter=iters, fuse_derivs=0, **opts), strict=strict)
        s.init(x0, u0)
        hist = []
        for it in range(iters):
            s.iterate(1)
            hist.append((s.ints("alpha_idx").copy(), s.ints("accepted").copy(), s.scalar("cost").copy(),
                         s.scalar("new_cost").copy(), s.scalar("lambda").copy()))
            if it == 2:
                s.x()  # a host read in the middle: the current trajectories go back to X / U and the solve goes on
        out = (hist, s.x(), s.u())
        s.close()
        family = 2 if opts.get("ls_keep", 2) == 2 else 1
        if family not in ref:
            ref[family] = out
            idx = np.concatenate([h[0] for h in hist])
            assert idx.max() >= 4  # with splits below 4 the second stage is exercised
        for fam, r in ref.items():
            exact = strict or fam == family
            same = np.array_equal if exact else close
            for h, hr in zip(out[0], r[0]):
                assert np.array_equal(h[0], hr[0]) and np.array_equal(h[1], hr[1]), opts  # step index, accepted: always
                for a, q in zip(h[2:], hr[2:]):
                    assert same(a, q), (opts, fam)
            assert same(out[1], r[1]) and same(out[2], r[2]), (opts, fam)


@pytest.mark.parametrize("fd", [0, 1])
def test_backward_pass_bit_exact_without_fma(ilqg, fd):
    """-ffp-contract=off build: the backward kernel reproduces the reference's gains BIT FOR BIT
    from the reference's derivative records (same operation order, IEEE sqrt/divide) — the
    only source of the 1e-10-level differences of the product build is FMA contraction."""
    g = golden("car_single_fd%d.npz" % fd)
    s = ilqg.BatchSolver("carparking", fd, batch=1, n_hor=500, params=ilqg.CAR_PARAMS, strict=True)
    s.init(g["x0"][None], g["u0"][None])
    for tag, lam in (("", float(g["lam"])), ("it12_", float(g["it12_lam"]))):
        u = g["u_nom"] if tag == "" else g["it12_u"]
        s.lib.ilqg_batch_set_u(s.h, np.ascontiguousarray(u[None]))
        s.set_derivs(g[tag + "rec"][None], g[tag + "fin"][None])
        s.set_scalar("lambda", lam)
        s.back_pass(single_sweep=True)
        l, L = s.gains()
        assert np.array_equal(l[0], g[tag + "l"]) and np.array_equal(L[0], g[tag + "L"])
        assert s.scalar("dV0")[0] == g[tag + "dV"][0] and s.scalar("dV1")[0] == g[tag + "dV"][1]
        assert s.scalar("g_norm")[0] == float(g[tag + "g_norm"])
    s.close()


# ---------------------------------------------------------------------------
# lock-step batch against the reference's 20-iteration fixture (the benchmark window)
# ---------------------------------------------------------------------------
def test_lockstep20_teacher_forced(ilqg, oracle_built):
    """The benchmark window (first 20 iterations), iteration by iteration.

    The iLQG iteration map amplifies rounding differences (SURVEY.md §7 hard part E): run
    freely, GPU and CPU agree to 1e-9 after 5 iterations but have drifted apart by iteration
    20 (different accepted step sizes), and meet again at convergence.  To pin every one of the
    20 iterations tightly, the GPU is re-synchronised with the oracle's nominal trajectory
    before each iteration and must then reproduce the oracle's NEXT state: same accepted
    step-size index, same lambda, cost and trajectory."""
    g = golden("car_lockstep20_fd0.npz")
    pick = [0, 7, 21, 40, 63]
    iters = int(g["iters"])
    x0, u0 = g["x0"][pick], g["u0"][pick]
    B = len(pick)

    def oracle_state(b, n_it):
        d = Driver(lib_path("oracle", full_ddp=0), 500, CAR_PARAMS, dict(max_iter=n_it))
        assert d.init(x0[b], u0[b]) == 1
        if n_it:
            d.solve()
        sc, (x, u), tr = d.scalars(), d.traj(0), d.trace()
        d.close()
        return sc, x, u, tr

    s = ilqg.BatchSolver("carparking", 0, batch=B, n_hor=500, params=ilqg.CAR_PARAMS, opts=dict(max_iter=iters + 1))
    s.init(x0, u0)
    states = [[oracle_state(b, it) for b in range(B)] for it in range(iters + 1)]
    for it in range(iters):
        s.set_x(np.array([states[it][b][1] for b in range(B)]))
        s.set_u(np.array([states[it][b][2] for b in range(B)]))
        s.set_scalar("cost", np.array([states[it][b][0]["cost"] for b in range(B)]))
        s.iterate(1)
        cost, lam, aidx, x = s.scalar("cost"), s.scalar("lambda"), s.ints("alpha_idx"), s.x()
        for b in range(B):
            sc, xr, ur, tr = states[it + 1][b]
            assert aidx[b] == tr["alpha_idx"][it], (it, b)
            assert close(lam[b], sc["lambda"], 1e-12), (it, b)
            assert close(cost[b], sc["cost"], 1e-9), (it, b, cost[b], sc["cost"])
            assert np.abs(x[b] - xr).max() < 1e-7, (it, b)
    s.close()


def test_lockstep20_free_running(ilqg):
    """free-running 20 iterations against the reference fixture: identical control flow counters,
    every cost decreased, and the batch statistics agree although individual paths have drifted"""
    g = golden("car_lockstep20_fd0.npz")
    B = len(g["cost"])
    s = ilqg.BatchSolver("carparking", 0, batch=B, n_hor=500, params=ilqg.CAR_PARAMS, opts=dict(max_iter=int(g["iters"])))
    s.init(g["x0"], g["u0"])
    c0 = s.scalar("cost")
    s.solve()
    assert np.array_equal(s.ints("iterations"), g["iterations"])
    assert np.array_equal(s.success(), g["rc"])
    cost = s.scalar("cost")
    assert np.all(cost < c0)
    rel = np.abs(cost - g["cost"]) / g["cost"]
    assert np.median(rel) < 0.05 and abs(cost.mean() / g["cost"].mean() - 1) < 0.02, (np.median(rel), cost.mean(), g["cost"].mean())
    s.close()


# ---------------------------------------------------------------------------
# full solves: batch path and the reference's drop-in iLQG() on the device
# ---------------------------------------------------------------------------
def test_full_solves_golden(ilqg):
    """16 full solves (65-365 iterations) against the reference's.  The iteration map amplifies rounding differences
    (see test_lockstep20_teacher_forced for the per-iteration statement), so the yardstick is the reference ITSELF:
    the fixture also holds the same solves by the reference built with FMA contraction (gcc -O3 -march=native), and
    the GPU may be as far from the FMA-free reference as that second CPU build is — measured: the two CPU builds
    differ by up to 1.5e-5 in final cost and 5e-2 in state (different iteration counts on 15 of 16 starts), the GPU by
    the same amounts on the same starts."""
    g = golden("car_solves_fd0.npz")
    B = len(g["rc"])
    s = ilqg.BatchSolver("carparking", 0, batch=B, n_hor=500, params=ilqg.CAR_PARAMS, opts=dict(max_iter=int(g["max_iter"])))
    s.init(g["x0"], g["u0"])
    s.solve()
    assert s.active() == 0
    assert np.array_equal(s.success(), g["rc"])
    cost, x = s.scalar("cost"), s.x()
    rel, rel_cpu = np.abs(cost / g["cost"] - 1), np.abs(g["fma_cost"] / g["cost"] - 1)
    dx, dx_cpu = np.abs(x - g["x"]).max(axis=(1, 2)), np.abs(g["fma_x"] - g["x"]).max(axis=(1, 2))
    de, de_cpu = np.abs(x[:, -1] - g["x"][:, -1]).max(axis=1), np.abs(g["fma_x"][:, -1] - g["x"][:, -1]).max(axis=1)
    assert np.all(np.isfinite(cost))
    # final cost: worst case and typical case no further off than between the two CPU builds (x3 for the sample of 16)
    assert rel.max() <= 3 * rel_cpu.max() and np.median(rel) <= 3 * np.median(rel_cpu), (rel, rel_cpu)
    # SURVEY 8(c)'s 1e-6 on the final cost holds for as many starts as it does between the CPU builds (one spare)
    assert np.sum(rel <= 2e-6) >= np.sum(rel_cpu <= 1e-6) - 1, (rel, rel_cpu)
    # trajectories (flat directions of the cost: the car may swing wider for the same cost) and the parked end state
    assert dx.max() <= 2 * dx_cpu.max() and np.median(dx) <= 3 * np.median(dx_cpu), (dx, dx_cpu)
    assert de.max() <= 2 * de_cpu.max(), (de, de_cpu)
    # where a start is insensitive (the CPU builds agree to 1e-9 in cost) the GPU agrees to the SURVEY tolerances
    calm = rel_cpu <= 1e-9
    assert np.all(rel[calm] <= 1e-6) and np.all(dx[calm] <= 1e-4), (rel[calm], dx[calm])
    s.close()


def test_multi_gpu_single_process(ilqg, synth):
    """ilqg_multi_*: the batch sharded over the GPUs of the node in one process, costs by ONE RCCL gather — equal to the
    single-GPU batch bit for bit (trajectories are independent).  Uses two devices where the box has them; with one
    device the same code runs as a communicator of one rank (ncclCommInitAll, ncclGather and the host hand-over)."""
    ndev = min(2, ilqg.Problem("carparking", 0).device_count())
    B, iters = 150, 4
    x0, u0 = synth.car_batch(B, first=300)
    one = ilqg.BatchSolver("carparking", 0, batch=B, n_hor=500, params=ilqg.CAR_PARAMS, opts=dict(max_iter=iters))
    one.init(x0, u0)
    one.iterate(iters)
    m = ilqg.MultiSolver("carparking", 0, batch=B, n_hor=500, devices=list(range(ndev)), params=ilqg.CAR_PARAMS,
                         opts=dict(max_iter=iters))
    assert m.devices() == ndev
    m.init(x0, u0)
    m.iterate(iters)
    assert np.array_equal(m.costs(), one.scalar("cost"))
    assert np.array_equal(m.x(), one.x()) and np.array_equal(m.ints("alpha_idx"), one.ints("alpha_idx"))
    assert m.active() == one.active()
    m.close()
    one.close()


def test_eight_shards_rehearsed_on_one_device(ilqg, synth):
    """BASELINE config 4's plumbing without the 8-GPU node: ilqg_multi_* with EIGHT shards, all on device 0 (a device
    list of equal ids: the same sharding, offsets, per-shard contexts and streams, send buffers and host hand-over;
    the gather is device-to-device copies instead of ncclGather).  A ragged last shard (1 000 = 7 x 125 + 125 -> use
    1 003: 7 x 126 + 121), parameters and options fanned out to every shard, costs / states / step indices equal to
    the single batch bit for bit; and what one host thread needs to enqueue one iteration of all eight shards."""
    import time
    B, iters, G = 1003, 4, 8
    x0, u0 = synth.car_batch(B, first=77)
    one = ilqg.BatchSolver("carparking", 0, batch=B, n_hor=500, params=ilqg.CAR_PARAMS, opts=dict(max_iter=iters + 8))
    one.init(x0, u0)
    one.iterate(iters)
    m = ilqg.MultiSolver("carparking", 0, batch=B, n_hor=500, devices=[0] * G, params=ilqg.CAR_PARAMS,
                         opts=dict(max_iter=iters + 8))
    assert m.devices() == G
    m.init(x0, u0)
    m.iterate(iters)
    assert np.array_equal(m.costs(), one.scalar("cost"))
    assert np.array_equal(m.x(), one.x()) and np.array_equal(m.u(), one.u())
    assert np.array_equal(m.ints("alpha_idx"), one.ints("alpha_idx")) and np.array_equal(m.ints("iterations"), one.ints("iterations"))
    assert m.active() == one.active()
    # host side of one iteration of all eight shards (launches and events only; the streams are idle when it starts)
    enq = []
    for _ in range(4):
        m.sync()
        t0 = time.perf_counter()
        m.iterate(1)
        enq.append(time.perf_counter() - t0)
        m.sync()
    print("host enqueue of one iteration, 8 shards: %.3f ms" % (1e3 * min(enq)))
    assert min(enq) < 3.5e-3  # half of a 7 ms iteration: one host thread can feed eight devices
    m.close()
    one.close()


def test_mex_entry_without_mex(ilqg, oracle_built):
    """ilqg_solve_single = the call sequence of the reference's MEX entry (iLQG_mex.c:55-137) on the product's drop-in
    iLQG(): same solve as the oracle's, the MEX entry's messages for refused arguments"""
    g = golden("car_single_fd0.npz")
    r = ilqg.solve_single(g["x0"], g["u0"], ilqg.CAR_PARAMS, dict(max_iter=6))
    o = Driver(lib_path("oracle", full_ddp=0), 500, CAR_PARAMS, dict(max_iter=6))
    assert o.init(g["x0"], g["u0"]) == 1
    o.solve()
    assert r["iterations"] == o.scalars()["iterations"] and close(r["cost"], o.scalars()["cost"], 1e-9)
    assert close(r["x"], o.traj(0)[0], 1e-8) and close(r["u"], o.traj(0)[1], 1e-8)
    assert r["seconds"] > 0
    o.close()
    with pytest.raises(ilqg.IlqgError, match="Parameter name 'cf' is not member of parameters struct"):
        ilqg.solve_single(g["x0"], g["u0"], {k: v for k, v in ilqg.CAR_PARAMS.items() if k != "cf"})
    with pytest.raises(ilqg.IlqgError, match="Parameter name 'pf' must be a vector length 4"):
        ilqg.solve_single(g["x0"], g["u0"], dict(ilqg.CAR_PARAMS, pf=[1.0, 2.0]))
    with pytest.raises(ilqg.IlqgError, match="Error setting optimization parameter 'zMin': parameter must be in range"):
        ilqg.solve_single(g["x0"], g["u0"], ilqg.CAR_PARAMS, dict(zMin=2.0))


# ---------------------------------------------------------------------------
# state-dependent input limits and regType 2
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("fd", [0, 1])
def test_state_dependent_limits_golden(ilqg, fd):
    """problems/hxtest: limits that depend on the state put the constraint gradients into the
    feedback gains (back_pass.c:186-199); device record carries *_sign and *_hx here"""
    check_hxtest_golden(ilqg, "hxtest", fd)


def check_hxtest_golden(ilqg, problem, fd):
    g = golden("hxtest_fd%d.npz" % fd)
    s = ilqg.BatchSolver(problem, fd, batch=1, n_hor=HX_N, params=HX_PARAMS, opts=dict(ls_split=0))
    assert s.problem.state_dep_limits == 1 and s.problem.rec_dev == s.problem.rec_host
    s.init(g["x0"][:1], g["u0"][:1])
    for tag in ("", "it3_"):
        s.set_x(g[tag + "x_nom"][None]); s.set_u(g[tag + "u_nom"][None])
        s.set_scalar("cost", float(g[tag + "cost"]))
        s.set_ints("need_derivs", 1)
        s.calc_derivs()
        rec, fin = s.derivs()
        assert close(rec[0], g[tag + "rec"]), worst(rec[0], g[tag + "rec"])
        s.set_scalar("lambda", float(g[tag + "lam"]))
        s.back_pass(single_sweep=True)
        assert s.ints("bp_rc")[0] == int(g[tag + "bp_rc"])
        l, L = s.gains()
        assert close(l[0], g[tag + "l"]) and close(L[0], g[tag + "L"]), (worst(l[0], g[tag + "l"]), worst(L[0], g[tag + "L"]))
        assert close(s.scalar("dV0")[0], g[tag + "dV"][0]) and close(s.scalar("g_norm")[0], g[tag + "g_norm"])
        # fused path: same gains from (x,u) directly
        s.set_scalar("lambda", float(g[tag + "lam"])); s.set_scalar("dlambda", 1.0)
        s.back_pass(fused=True)
        l2, L2 = s.gains()
        assert close(l2[0], g[tag + "l"]) and close(L2[0], g[tag + "L"])
        s.set_scalar("lambda", float(g[tag + "lam"]))
        s.line_search()
        assert s.ints("accepted")[0] == int(g[tag + "ls_accept"]) and s.ints("alpha_idx")[0] == int(g[tag + "ls_index"])
        assert close(s.scalar("new_cost")[0], g[tag + "new_cost"], 1e-9)
        assert close(s.x()[0], g[tag + "x_cand"], 1e-9) and close(s.u()[0], g[tag + "u_cand"], 1e-9)
    s.close()
    B = len(g["solve_rc"])
    s = ilqg.BatchSolver(problem, fd, batch=B, n_hor=HX_N, params=HX_PARAMS, opts=dict(max_iter=100))
    s.init(g["x0"], g["u0"])
    s.solve()
    assert np.array_equal(s.success(), g["solve_rc"]) and np.array_equal(s.ints("iterations"), g["solve_iterations"])
    assert close(s.scalar("cost"), g["solve_cost"], 1e-8) and np.abs(s.x() - g["solve_x"]).max() < 1e-4
    s.close()


@pytest.mark.parametrize("fd", [0, 1])
def test_regtype2_golden(ilqg, fd):
    # (at FULL_DDP = 1 the reference abandons this sweep — fd1_rc == 1 — and only the return code is compared here: the
    # gains of completed and of abandoned regType-2 sweeps, in every mapping, are held by tests/test_gpu_regtype2.py)
    g = golden("car_regtype2.npz")
    s = ilqg.BatchSolver("carparking", fd, batch=1, n_hor=500, params=ilqg.CAR_PARAMS, opts=dict(regType=2))
    s.init(g["x0"][None], g["u0"][None])
    s.calc_derivs()
    s.set_scalar("lambda", 1.0)
    s.back_pass(single_sweep=True)
    assert s.ints("bp_rc")[0] == int(g["fd%d_rc" % fd])
    if int(g["fd%d_rc" % fd]) == 0:
        l, L = s.gains()
        assert close(l[0], g["fd%d_l" % fd]) and close(L[0], g["fd%d_L" % fd])
        assert close(s.scalar("dV0")[0], g["fd%d_dV" % fd][0]) and close(s.scalar("g_norm")[0], g["fd%d_g_norm" % fd])
    s.close()


# ---------------------------------------------------------------------------
# wave mapping (one wavefront per trajectory): n=16/m=8 synthetic problem, and CarParking forced into it
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("fd,variant", [(0, ""), (1, ""), (0, "_plain"), (1, "_plain"), (1, "p")])
def test_wave_mapping_synthetic_golden(ilqg, fd, variant):
    """variant "_plain": the same problem emitted without hints or tables; "p": synth16p, the n = 16 problem whose
    tensors do not factor (pairwise state products in the nonlinearity) — both take the stored-tensor path"""
    problem = "synth16p" if variant == "p" else "synth16x8" + variant
    g = golden("%s_fd%d.npz" % ("synth16p" if variant == "p" else "synth16x8", fd))
    N = int(g["n_hor"])
    SYN_PARAMS_TIGHT = SYNP_PARAMS_TIGHT if variant == "p" else SYN_TIGHT
    s = ilqg.BatchSolver(problem, fd, batch=1, n_hor=N, params=SYN_PARAMS_TIGHT, opts=dict(ls_split=0))
    assert s.problem.wave_mapping and (s.problem.nx, s.problem.nu) == (16, 8)
    s.init(g["x0"][:1], g["u0"][:1])
    assert close(s.scalar("cost")[0], g["cost"])
    for tag in ("", "it3_"):
        s.set_x(g[tag + "x_nom"][None]); s.set_u(g[tag + "u_nom"][None])
        s.set_scalar("cost", float(g[tag + "cost"]))
        s.calc_derivs()
        rec, fin = s.derivs()
        assert close(rec[0], g[tag + "rec"]), worst(rec[0], g[tag + "rec"])
        assert close(fin[0], g[tag + "fin"])
        s.set_scalar("lambda", float(g[tag + "lam"]))
        s.back_pass(single_sweep=True)
        assert s.ints("bp_rc")[0] == int(g[tag + "bp_rc"]) == 0
        l, L = s.gains()
        assert close(l[0], g[tag + "l"]), worst(l[0], g[tag + "l"])
        assert close(L[0], g[tag + "L"]), worst(L[0], g[tag + "L"])
        assert close(s.scalar("dV0")[0], g[tag + "dV"][0]) and close(s.scalar("dV1")[0], g[tag + "dV"][1])
        assert close(s.scalar("g_norm")[0], g[tag + "g_norm"])
        s.line_search()
        assert s.ints("accepted")[0] == int(g[tag + "ls_accept"]) and s.ints("alpha_idx")[0] == int(g[tag + "ls_index"])
        assert close(s.scalar("new_cost")[0], g[tag + "new_cost"], 1e-9)
        assert close(s.x()[0], g[tag + "x_cand"], 1e-9) and close(s.u()[0], g[tag + "u_cand"], 1e-9)
    s.close()
    # lock-step batch (ragged size) against the oracle, derivative records chunked through the work buffer
    B, iters = 5, 4
    x0, u0 = syn_inputs(B, N, first=40)
    s = ilqg.BatchSolver(problem, fd, batch=B, n_hor=N, params=SYN_PARAMS_TIGHT, opts=dict(max_iter=iters))
    s.init(x0, u0)
    s.iterate(iters)
    cost, x = s.scalar("cost"), s.x()
    for b in range(B):
        d = Driver(lib_path("oracle", "synth16p" if variant == "p" else "synth16x8", fd), N, SYN_PARAMS_TIGHT, dict(max_iter=iters))
        assert d.init(x0[b], u0[b]) == 1
        d.solve()
        assert close(cost[b], d.scalars()["cost"], 1e-9), (b, cost[b], d.scalars()["cost"])
        assert np.abs(x[b] - d.traj(0)[0]).max() < 1e-7
        d.close()
    s.close()


@pytest.mark.parametrize("fd", [0, 1])
@pytest.mark.parametrize("strict", [True, False])
def test_quad_mapping_equals_the_row_mapping(ilqg, monkeypatch, fd, strict):
    """The backward pass with 16 lanes per trajectory (ilqg_quad.hpp: four trajectories per wavefront, every 16-lane row
    at its own step, sweep and lambda) against the one-wavefront-per-trajectory row mapping (ILQG_NO_QUAD=1) on a ragged
    batch whose trajectories need different numbers of sweeps: gains, value changes, gradient norms, lambdas, sweep counts
    and the solves that follow — the same bits in the FMA-free build, to the single-pass tolerance in the product build"""
    B, N, K = 37, 300, 4
    x0, u0 = syn_inputs(B, N, first=7)
    x0 = x0 * np.linspace(0.2, 3.0, B)[:, None]  # spread: some starts need lambda retries, some none

    def run():
        # (a small initial lambda: the first sweeps of some trajectories meet an indefinite Quu and are abandoned)
        s = ilqg.BatchSolver("synth16x8", fd, batch=B, n_hor=N, params=SYN_PARAMS, opts=dict(max_iter=K + 1, lambdaInit=1e-7), strict=strict)
        s.init(x0, u0)
        out = []
        for it in range(K):
            s.back_pass(fused=True)
            l, L = s.gains()
            out.append(dict(l=l.copy(), L=L.copy(), dV0=s.scalar("dV0").copy(), dV1=s.scalar("dV1").copy(), g=s.scalar("g_norm").copy(),
                            lam=s.scalar("lambda").copy(), calls=s.ints("bp_calls").copy(), rc=s.ints("bp_rc").copy()))
            s.line_search()
            s.update()
        out.append(dict(cost=s.scalar("cost").copy(), x=s.x().copy()))
        s.close()
        return out

    quad = run()
    monkeypatch.setenv("ILQG_NO_QUAD", "1")
    row = run()
    calls = np.concatenate([o["calls"] for o in quad[:-1]])
    assert calls.min() == 1 and (fd == 0 or calls.max() > 1), np.bincount(calls)
    for it, (a, b) in enumerate(zip(quad, row)):
        for k in a:
            if strict or k in ("calls", "rc"):
                assert np.array_equal(a[k], b[k]), k
            else:
                # product builds: the two mappings contract differently (FMA; the quad mapping's product build also takes
                # ONE of the reference's two half sums of a symmetric product) — the single-pass bar of DESIGN §4 for the
                # first pass, then the free-running iterations amplify the difference
                tol = 1e-10 if it == 0 else 1e-7
                assert np.all(np.abs(a[k] - b[k]) <= tol * np.maximum(1.0, np.abs(b[k]))), (it, k, np.abs(a[k] - b[k]).max())


@pytest.mark.parametrize("strict", [True, False])
def test_derivative_records_in_parts_equal_the_per_lane_ones(ilqg, monkeypatch, strict):
    """k_derivs_parts (ILQG_DERIV_PARTS=1: the time-varying record entries from the generated file's PARTS — auxiliaries,
    sin / cos once, products, 16 outputs at a time through an LDS tile, whole lines out) against k_derivs_wave (the
    generated code on a struct per lane): the solves that consume the records — gains, value changes, accepted steps,
    costs — the same bits in the FMA-free build, to rounding in the product build"""
    B, N, K = 70, 200, 4
    x0, u0 = syn_inputs(B, N, first=3)

    def run():
        s = ilqg.BatchSolver("synth16x8", 1, batch=B, n_hor=N, params=SYN_PARAMS, opts=dict(max_iter=K + 1), strict="exp_strict" if strict else "exp")
        s.init(x0, u0)
        out = []
        for it in range(K):
            s.iterate(1)
            l, L = s.gains()
            out.append(dict(l=l.copy(), L=L.copy(), dV0=s.scalar("dV0").copy(), g=s.scalar("g_norm").copy(), cost=s.scalar("cost").copy(),
                            idx=s.ints("alpha_idx").copy(), status=s.ints("status").copy()))
        s.close()
        return out

    plain = run()
    monkeypatch.setenv("ILQG_DERIV_PARTS", "1")
    parts = run()
    assert all((o["status"] == 0).all() for o in parts)
    for a, b in zip(plain, parts):
        for k in a:
            if strict or k in ("idx", "status"):
                assert np.array_equal(a[k], b[k]), k
            else:
                assert np.allclose(a[k], b[k], rtol=1e-8, atol=1e-11), (k, np.abs(a[k] - b[k]).max())


@pytest.mark.parametrize("log2_scale", [-240, -120, 0, 120, 240])
def test_wave_mapping_step_with_scaled_costs(ilqg, oracle_built, log2_scale):
    """The row-mapped backward step takes short forms of sqrt / reciprocal / quotient in its box QP while the pivots lie
    in [2^-200, 2^200] and the compiler's general ones otherwise (ilqg_row.hpp).  With every cost weight scaled by
    2^+-120 (and lambda with them) the short forms work on large and small numbers, with 2^+-240 the general ones run:
    the FMA-free build must give the oracle's gains bit for bit either way (stored derivative records of the oracle, so
    that nothing but the backward step is compared)."""
    N, fd = 12, 1
    sc = 2.0 ** log2_scale
    params = dict(SYN_PARAMS_TIGHT)
    for k in ("ru", "qx", "qf"):
        params[k] = [v * sc for v in params[k]]
    x0, u0 = syn_inputs(1, N, first=7)
    d = Driver(lib_path("oracle", "synth16x8", fd), N, params, {})
    assert d.init(x0[0], u0[0]) == 1
    assert d.calc_derivs() == 1
    lam = sc
    d.set_lambda(lam)
    rc = d.back_pass()
    rec, fin = d.derivs()
    l0, L0 = d.gains()
    d.close()
    # (with the large scales the reference's box QP gives up at the first step it meets — its absolute thresholds — and
    # the sweep is abandoned: then the same has to happen here, and the gains of the steps behind it have to agree)
    assert rc == (0 if log2_scale <= 0 else 1)
    s = ilqg.BatchSolver("synth16x8", fd, batch=1, n_hor=N, params=params, strict=True, opts=dict(fuse_derivs=0))
    s.init(x0, u0)
    s.set_derivs(rec[None], fin[None])
    s.set_scalar("lambda", lam)
    s.back_pass(single_sweep=True)
    assert s.ints("bp_rc")[0] == rc
    l, L = s.gains()
    done = slice(None) if rc == 0 else slice(N - 1, N)  # an abandoned sweep: the last step was the first to be met
    if rc == 0 or np.any(l0[N - 1] != 0) or np.any(L0[N - 1] != 0):
        assert np.array_equal(l[0][done], l0[done]) and np.array_equal(L[0][done], L0[done]), (worst(l[0], l0), worst(L[0], L0))
    s.close()
    if rc:
        return
    # and with the records of the device's own derivative kernel (factored tensors): gains within rounding of the oracle's
    s = ilqg.BatchSolver("synth16x8", fd, batch=1, n_hor=N, params=params, strict=True)
    s.init(x0, u0)
    s.calc_derivs()
    s.set_scalar("lambda", lam)
    s.back_pass(single_sweep=True)
    l, L = s.gains()
    assert s.ints("bp_rc")[0] == 0 and close(l[0], l0, 1e-9) and close(L[0], L0, 1e-9)
    s.close()


def test_wave_mapping_element_step(ilqg):
    """The backward step of the wave mapping for problems whose rows do not fit a 16-lane DPP row (N_X > 16 or N_U > 16:
    one OUTPUT element per lane, both operands from LDS; ilqg_wave.hpp back_step_wave) — compiled for the n = 16 problem
    with -DILQG_ROW_STEP=0 (libilqg_synth16x8_fd1_hip_elem.so, FMA-free) so that the path is exercised although no
    shipped problem is that large: the reference's goldens at the single-pass tolerance, and bit for bit the results of
    the row-mapped FMA-free build (both keep the reference's order of operations), stored tensors, over whole
    iterations with lambda retries."""
    g = golden("synth16x8_fd1.npz")
    N = int(g["n_hor"])
    s = ilqg.BatchSolver("synth16x8", 1, batch=1, n_hor=N, params=SYN_PARAMS_TIGHT, opts=dict(ls_split=0), strict="elem")
    s.init(g["x0"][:1], g["u0"][:1])
    for tag in ("", "it3_"):
        s.set_x(g[tag + "x_nom"][None]); s.set_u(g[tag + "u_nom"][None])
        s.set_scalar("cost", float(g[tag + "cost"]))
        s.calc_derivs()
        s.set_scalar("lambda", float(g[tag + "lam"]))
        s.back_pass(single_sweep=True)
        assert s.ints("bp_rc")[0] == int(g[tag + "bp_rc"]) == 0
        l, L = s.gains()
        assert close(l[0], g[tag + "l"]), worst(l[0], g[tag + "l"])
        assert close(L[0], g[tag + "L"]), worst(L[0], g[tag + "L"])
        assert close(s.scalar("dV0")[0], g[tag + "dV"][0]) and close(s.scalar("dV1")[0], g[tag + "dV"][1])
        assert close(s.scalar("g_norm")[0], g[tag + "g_norm"])
    s.close()
    B, iters = 9, 4
    x0, u0 = syn_inputs(B, N, first=11)
    out = []
    for build in (True, "elem"):
        s = ilqg.BatchSolver("synth16x8", 1, batch=B, n_hor=N, params=SYN_PARAMS_TIGHT, opts=dict(max_iter=iters, fuse_derivs=0, lambdaInit=1e-3),
                             strict=build)
        s.init(x0, u0)
        s.iterate(iters)
        out.append((s.scalar("cost"), s.x(), s.ints("bp_calls"), s.ints("alpha_idx")))
        s.close()
    for a, b in zip(*out):
        assert np.array_equal(a, b)


@pytest.mark.parametrize("strict", [False, True])
def test_factored_tensors_equal_stored_tensors(ilqg, strict):
    """n=16 FULL_DDP: the backward pass that multiplies the tensors out of the generated coefficient tables (records
    carry the 32 products of a step; option fuse_derivs) against the one that reads fxx/fuu/fxu from the records.
    Same products in the same order: bit-identical without FMA contraction.  B = 9: the workgroups that share the
    tables hold several trajectories, the last one is partly filled."""
    g = golden("synth16x8_fd1.npz")
    N = int(g["n_hor"])
    B, iters = 9, 4
    x0, u0 = syn_inputs(B, N, first=200)
    res = []
    for fuse in (0, 1):
        s = ilqg.BatchSolver("synth16x8", 1, batch=B, n_hor=N, params=SYN_PARAMS_TIGHT,
                             opts=dict(max_iter=iters, fuse_derivs=fuse), strict=strict)
        s.init(x0, u0)
        s.iterate(iters)
        l, L = s.gains()
        res.append((s.scalar("cost"), s.x(), s.u(), l, L, s.scalar("lambda"), s.ints("alpha_idx"), s.ints("bp_calls")))
        s.close()
    a, b = res
    assert np.array_equal(a[6], b[6]) and np.array_equal(a[7], b[7])
    for va, vb in zip(a[:6], b[:6]):
        if strict:
            assert np.array_equal(va, vb), worst(va, vb)
        else:
            assert close(va, vb, 1e-9), worst(va, vb)


def test_wave_mapping_chunked_records(ilqg, monkeypatch):
    """a work buffer smaller than the batch: derivative records are produced and consumed chunk by chunk"""
    g = golden("synth16x8_fd0.npz")
    N = int(g["n_hor"])
    B, iters = 7, 3
    x0, u0 = syn_inputs(B, N, first=80)
    out = []
    for gb in ("24", "0.002"):  # 0.002 GB ~ 6 trajectories of 32 steps x 9.5 KB -> two chunks
        monkeypatch.setenv("ILQG_WORK_GB", gb)
        s = ilqg.BatchSolver("synth16x8", 0, batch=B, n_hor=N, params=SYN_PARAMS_TIGHT, opts=dict(max_iter=iters))
        s.init(x0, u0)
        s.iterate(iters)
        out.append((s.scalar("cost"), s.x(), s.ints("alpha_idx")))
        s.close()
    assert np.array_equal(out[0][0], out[1][0]) and np.array_equal(out[0][1], out[1][1]) and np.array_equal(out[0][2], out[1][2])


def test_wave_mapping_carparking(ilqg, synth):
    """CarParking in the one-wavefront-per-trajectory mapping (BASELINE config 2 wording): same gains as the
    reference, same iterations as the lane mapping"""
    g = golden("car_single_fd0.npz")
    s = ilqg.BatchSolver("carparking", 0, batch=1, n_hor=500, params=ilqg.CAR_PARAMS, opts=dict(ls_split=0), strict="wave")
    assert s.problem.wave_mapping
    s.init(g["x0"][None], g["u0"][None])
    s.calc_derivs()
    s.back_pass(single_sweep=True)
    l, L = s.gains()
    assert close(l[0], g["l"]) and close(L[0], g["L"]), (worst(l[0], g["l"]), worst(L[0], g["L"]))
    assert close(s.scalar("dV0")[0], g["dV"][0]) and close(s.scalar("g_norm")[0], g["g_norm"])
    s.line_search()
    assert s.ints("alpha_idx")[0] == int(g["ls_index"]) and close(s.scalar("new_cost")[0], g["new_cost"])
    s.close()
    B, iters = 70, 4
    x0, u0 = synth.car_batch(B, first=2000)
    res = []
    for mode in (False, "wave"):
        s = ilqg.BatchSolver("carparking", 0, batch=B, n_hor=500, params=ilqg.CAR_PARAMS, opts=dict(max_iter=iters), strict=mode)
        s.init(x0, u0)
        s.iterate(iters)
        res.append((s.scalar("cost"), s.ints("alpha_idx"), s.x()))
        s.close()
    assert close(res[0][0], res[1][0], 1e-9) and np.array_equal(res[0][1], res[1][1]) and np.abs(res[0][2] - res[1][2]).max() < 1e-7


# ---------------------------------------------------------------------------
# randomised batch vs oracle, ragged batch size, properties at full size
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("fd,B", [(0, 97), (1, 33)])
def test_random_batch_vs_oracle(ilqg, synth, oracle_built, fd, B):
    """B is not a multiple of 64: the padded lanes must not disturb anything"""
    iters = 5
    x0, u0 = synth.car_batch(B, first=7000)
    s = ilqg.BatchSolver("carparking", fd, batch=B, n_hor=500, params=ilqg.CAR_PARAMS, opts=dict(max_iter=iters))
    s.init(x0, u0)
    s.iterate(iters)
    cost, lam, x, aidx = s.scalar("cost"), s.scalar("lambda"), s.x(), s.ints("alpha_idx")
    for b in list(range(0, B, 8)) + [B - 1]:
        d = Driver(lib_path("oracle", full_ddp=fd), 500, CAR_PARAMS, dict(max_iter=iters))
        assert d.init(x0[b], u0[b]) == 1
        d.solve()
        sc = d.scalars()
        assert close(cost[b], sc["cost"], 1e-9), (b, cost[b], sc["cost"])
        assert close(lam[b], sc["lambda"], 1e-12)
        assert aidx[b] == d.trace()["alpha_idx"][-1]
        assert np.abs(x[b] - d.traj(0)[0]).max() < 1e-7
        d.close()
    s.close()


@pytest.mark.parametrize("mapping", [False, "wave"])
def test_properties_at_benchmark_size(ilqg, synth, mapping):
    """B = 4096 (BASELINE config 2): size-independent properties instead of a CPU re-run — in the lane mapping (the
    product's choice for n = 4) and in the mapping the config names, one wavefront per trajectory"""
    B, iters = 4096, 4
    x0, u0 = synth.car_batch(B)
    s = ilqg.BatchSolver("carparking", 0, batch=B, n_hor=500, params=ilqg.CAR_PARAMS, opts=dict(max_iter=50), strict=mapping)
    assert s.problem.wave_mapping == (mapping == "wave")
    s.init(x0, u0)
    c0 = s.scalar("cost")
    # the initial roll-out clamps u into the box and keeps x0
    u = s.u()
    assert u[..., 0].min() >= -0.5 and u[..., 0].max() <= 0.5 and u[..., 1].min() >= -2.0 and u[..., 1].max() <= 2.0
    assert np.array_equal(s.x()[:, 0, :], x0)
    prev = c0
    for _ in range(iters):
        s.iterate(1)
        c = s.scalar("cost")
        acc = s.ints("accepted").astype(bool)
        # accepted steps strictly reduce the cost (zMin = 0), rejected ones leave it untouched
        assert np.all(c[acc] < prev[acc]) and np.array_equal(c[~acc], prev[~acc])
        prev = c
    # trajectory b of the big batch equals trajectory b solved alone (no cross-talk between lanes)
    small = ilqg.BatchSolver("carparking", 0, batch=3, n_hor=500, params=ilqg.CAR_PARAMS, opts=dict(max_iter=50), strict=mapping)
    pick = [5, 1000, 4095]
    small.init(x0[pick], u0[pick])
    small.iterate(iters)
    assert np.array_equal(small.scalar("cost"), prev[pick])
    assert np.array_equal(small.x(), s.x()[pick])
    if mapping == "wave":  # ... and the same three trajectories in the lane mapping: same steps, same results to rounding
        lane = ilqg.BatchSolver("carparking", 0, batch=3, n_hor=500, params=ilqg.CAR_PARAMS, opts=dict(max_iter=50))
        lane.init(x0[pick], u0[pick])
        lane.iterate(iters)
        assert np.array_equal(lane.ints("alpha_idx"), small.ints("alpha_idx"))
        assert close(lane.scalar("cost"), small.scalar("cost"), 1e-9) and np.abs(lane.x() - small.x()).max() < 1e-7
        lane.close()
    s.close(); small.close()


def test_properties_at_full_benchmark_batch(ilqg, synth, oracle_built):
    """B = 65 536 (BASELINE config 3, the batch the metric is quoted on; four stream groups by default): accepted
    steps reduce the cost, every trajectory is still active inside the window, trajectories picked from different
    groups and tiles equal the same trajectories solved alone, and one of them equals the CPU oracle."""
    B, iters = 65536, 3
    x0, u0 = synth.car_batch(B)
    s = ilqg.BatchSolver("carparking", 0, batch=B, n_hor=500, params=ilqg.CAR_PARAMS, opts=dict(max_iter=50))
    assert s.groups() == 4
    s.init(x0, u0)
    prev = s.scalar("cost")
    for _ in range(iters):
        s.iterate(1)
        c = s.scalar("cost")
        acc = s.ints("accepted").astype(bool)
        assert np.all(c[acc] < prev[acc]) and np.array_equal(c[~acc], prev[~acc])
        prev = c
    assert s.active() == B and np.all(s.ints("iterations") == iters)
    pick = [0, 15, 16, 63, 64, 16383, 16384, 40000, 49151, 49152, 65535]   # group (16 384), tile and search-wavefront (16) boundaries
    x_big, u_big = s.x()[pick], s.u()[pick]
    small = ilqg.BatchSolver("carparking", 0, batch=len(pick), n_hor=500, params=ilqg.CAR_PARAMS, opts=dict(max_iter=50))
    small.init(x0[pick], u0[pick])
    small.iterate(iters)
    assert np.array_equal(small.scalar("cost"), prev[pick])
    assert np.array_equal(small.x(), x_big) and np.array_equal(small.u(), u_big)
    d = Driver(lib_path("oracle", full_ddp=0), 500, CAR_PARAMS, dict(max_iter=iters))
    assert d.init(x0[40000], u0[40000]) == 1
    d.solve()
    assert close(prev[40000], d.scalars()["cost"], 1e-9)
    d.close(); s.close(); small.close()


def test_properties_at_config5_size_with_stored_tensors(ilqg, synth, oracle_built):
    """BASELINE config 5 at full size from the pair WITHOUT hints (synth16x8_plain: stored tensors, 47.9 KB records): the
    production path the fixture-sized tests (one piece of the record buffer) never reach — eight pieces per iteration on two
    streams, the derivative kernel of one piece (private element with proxies, 512-byte records: ilqgdev) beside the
    row-mapped backward kernel of the piece before it, constants written once per half of the buffer, the scalar
    roll-outs with the 7-row second stage.  Accepted steps reduce the cost and rejected ones leave it untouched;
    trajectories at piece boundaries and at the ends of the batch equal the same trajectories solved alone (one piece, no
    neighbour kernel), bit for bit, over two iterations and again after a third (records of the buffer reused with their
    constants in place); one of them equals the CPU oracle."""
    B, N, iters = 16384, 1000, 2
    x0, u0 = synth.synth16_batch(B, N)
    s = ilqg.BatchSolver("synth16x8_plain", 1, batch=B, n_hor=N, params=SYN_PARAMS, opts=dict(max_iter=50))
    assert s.problem.wave_mapping
    s.init(x0, u0)
    prev = s.scalar("cost")
    n_acc = 0
    for _ in range(iters):
        s.iterate(1)
        c = s.scalar("cost")
        acc = s.ints("accepted").astype(bool)
        assert np.all(c[acc] < prev[acc]) and np.array_equal(c[~acc], prev[~acc])
        n_acc += int(acc.sum())
        prev = c
    assert n_acc > B and np.all(s.ints("iterations") <= iters)
    pick = [0, 1, 2047, 2048, 2049, 4095, 4096, 8191, 8192, 12345, 14335, 14336, 16383]
    x2, u2, a2, c2 = s.x()[pick], s.u()[pick], s.ints("alpha_idx")[pick], prev[pick]
    s.iterate(1)
    x3, u3, c3, calls3 = s.x()[pick], s.u()[pick], s.scalar("cost")[pick], s.ints("bp_calls")[pick]
    s.close()
    small = ilqg.BatchSolver("synth16x8_plain", 1, batch=len(pick), n_hor=N, params=SYN_PARAMS, opts=dict(max_iter=50))
    small.init(x0[pick], u0[pick])
    small.iterate(iters)
    assert np.array_equal(small.scalar("cost"), c2) and np.array_equal(small.ints("alpha_idx"), a2)
    assert np.array_equal(small.x(), x2) and np.array_equal(small.u(), u2)
    small.iterate(1)
    assert np.array_equal(small.scalar("cost"), c3) and np.array_equal(small.ints("bp_calls"), calls3)
    assert np.array_equal(small.x(), x3) and np.array_equal(small.u(), u3)
    small.close()
    b = 12345
    d = Driver(lib_path("oracle", "synth16x8", 1), N, SYN_PARAMS, dict(max_iter=iters))
    assert d.init(x0[b], u0[b]) == 1
    d.solve()
    assert close(c2[pick.index(b)], d.scalars()["cost"], 1e-9), (c2[pick.index(b)], d.scalars()["cost"])
    assert np.abs(x2[pick.index(b)] - d.traj(0)[0]).max() < 1e-7
    d.close()


def test_properties_at_config5_size(ilqg, synth, oracle_built):
    """BASELINE config 5 at full size (synthetic n = 16, m = 8, N = 1000, FULL_DDP = 1, 16 384 trajectories): the
    production path of the wave mapping — two pieces of 8 192 trajectories on two streams, backward wavefronts taking
    trajectories from the queue, factored records lying overlapped in the device's work buffer, the 7-row second search
    stage — which the fixture-sized tests (B <= 150, N <= 40) never reach.  Accepted steps reduce the cost and rejected
    ones leave it untouched; trajectories at the piece boundary (8 191 / 8 192), at the first and last place of a
    backward workgroup (8 wavefronts) and at the ends of the batch equal the same trajectories solved alone, bit for
    bit; one of them equals the CPU oracle."""
    B, N, iters = 16384, 1000, 2
    x0, u0 = synth.synth16_batch(B, N)
    s = ilqg.BatchSolver("synth16x8", 1, batch=B, n_hor=N, params=SYN_PARAMS, opts=dict(max_iter=50))
    assert s.problem.wave_mapping
    s.init(x0, u0)
    prev = s.scalar("cost")
    n_acc = 0
    for _ in range(iters):
        s.iterate(1)
        c = s.scalar("cost")
        acc = s.ints("accepted").astype(bool)
        assert np.all(c[acc] < prev[acc]) and np.array_equal(c[~acc], prev[~acc])
        n_acc += int(acc.sum())
        prev = c
    assert n_acc > B and np.all(s.ints("iterations") <= iters)
    pick = [0, 7, 8, 8191, 8192, 8199, 12345, 16383]
    x_big, u_big = s.x()[pick], s.u()[pick]
    alpha_big = s.ints("alpha_idx")[pick]
    s.close()
    small = ilqg.BatchSolver("synth16x8", 1, batch=len(pick), n_hor=N, params=SYN_PARAMS, opts=dict(max_iter=50))
    small.init(x0[pick], u0[pick])
    small.iterate(iters)
    assert np.array_equal(small.scalar("cost"), prev[pick])
    assert np.array_equal(small.ints("alpha_idx"), alpha_big)
    assert np.array_equal(small.x(), x_big) and np.array_equal(small.u(), u_big)
    small.close()
    b = 12345
    d = Driver(lib_path("oracle", "synth16x8", 1), N, SYN_PARAMS, dict(max_iter=iters))
    assert d.init(x0[b], u0[b]) == 1
    d.solve()
    assert close(prev[b], d.scalars()["cost"], 1e-9), (prev[b], d.scalars()["cost"])
    assert np.abs(x_big[pick.index(b)] - d.traj(0)[0]).max() < 1e-7
    d.close()
    # ALL eight against the CPU oracle, three iterations at the full horizon, teacher forced: before iteration i the
    # product build (quad-mapped step: FMA contraction, one half sum of the symmetric products, the contraction's order,
    # DESIGN 2.2) gets the oracle's state after i iterations and must reproduce the oracle's iteration i + 1 — the gains
    # of its backward pass (the last sweep of the lambda retries) at the single-pass bar, the lambda they were made
    # with and the accepted step size exactly, cost and trajectory to rounding (back_pass.c:163-241, line_search.c:37-75)
    def oracle_after(bb, n_it):
        dd = Driver(lib_path("oracle", "synth16x8", 1), N, SYN_PARAMS, dict(max_iter=max(n_it, 1)))
        assert dd.init(x0[bb], u0[bb]) == 1
        if n_it:
            dd.solve()
        sc, (xx, uu), tr = dd.scalars(), dd.traj(0), dd.trace()
        dd.close()
        return sc, xx, uu, tr

    def oracle_first_gains(bb):
        """the gains of the first iteration's backward pass: sweeps from lambda = dlambda = 1 with the reference's retry
        schedule (iLQG.c:261-275) until one succeeds (the oracle's own solve() swaps the buffers, its gains are gone)"""
        dd = Driver(lib_path("oracle", "synth16x8", 1), N, SYN_PARAMS, dict(max_iter=1))
        assert dd.init(x0[bb], u0[bb]) == 1 and dd.calc_derivs() == 1
        lam, dlam, sweeps = 1.0, 1.0, 0
        while True:
            dd.set_lambda(lam)
            sweeps += 1
            if dd.back_pass() == 0:
                break
            dlam = max(dlam * 1.6, 1.6)
            lam = max(lam * dlam, 1e-6)
            assert lam <= 1e10
        ll, LL = dd.gains()
        dd.close()
        return ll, LL, lam, sweeps
    states = [[oracle_after(bb, i) for bb in pick] for i in range(4)]
    small = ilqg.BatchSolver("synth16x8", 1, batch=len(pick), n_hor=N, params=SYN_PARAMS, opts=dict(max_iter=50))
    small.init(x0[pick], u0[pick])
    worst_l = worst_L = 0.0
    for i in range(3):
        if i:
            small.set_x(np.array([st[1] for st in states[i]]))
            small.set_u(np.array([st[2] for st in states[i]]))
            small.set_scalar("cost", np.array([st[0]["cost"] for st in states[i]]))
            # (lambda / dlambda follow by themselves while the decisions agree — asserted below)
        small.iterate(1)
        l, L = small.gains()
        cost, lam, aidx, xg, calls = small.scalar("cost"), small.scalar("lambda"), small.ints("alpha_idx"), small.x(), small.ints("bp_calls")
        for j, bb in enumerate(pick):
            sc, xr, ur, tr = states[i + 1][j]
            assert aidx[j] == tr["alpha_idx"][i], (i, bb, aidx[j], tr["alpha_idx"][i])
            assert close(lam[j], sc["lambda"], 1e-12), (i, bb)
            assert calls[j] == tr["bp_calls"][i], (i, bb, calls[j], tr["bp_calls"][i])
            if i == 0:
                lr, Lr, _, sweeps = oracle_first_gains(bb)
                assert sweeps == calls[j] and close(l[j], lr) and close(L[j], Lr), (bb, sweeps, calls[j], worst(l[j], lr), worst(L[j], Lr))
                worst_l, worst_L = max(worst_l, worst(l[j], lr)), max(worst_L, worst(L[j], Lr))
            assert close(cost[j], sc["cost"], 1e-9), (i, bb, cost[j], sc["cost"])
            assert np.abs(xg[j] - xr).max() < 1e-7, (i, bb)
    small.close()
    print("config 5, product build against the oracle, first backward pass of 8 trajectories at N = 1000: worst deviation of l %.2e, of L %.2e" % (worst_l, worst_L))


def test_results_do_not_depend_on_stream_groups(ilqg, synth):
    """the batch advances as 1..4 groups of trajectories on separate HIP streams (ilqg_batch_create_groups):
    bit-identical results, ragged group sizes included"""
    B, iters = 1000, 6
    x0, u0 = synth.car_batch(B, first=123)
    ref = None
    for groups in (1, 2, 3, 4):
        s = ilqg.BatchSolver("carparking", 0, batch=B, n_hor=500, params=ilqg.CAR_PARAMS, opts=dict(max_iter=iters),
                             groups=groups)
        assert s.groups() == groups
        s.init(x0, u0)
        s.iterate(iters)
        out = (s.scalar("cost"), s.scalar("lambda"), s.x(), s.u(), s.ints("alpha_idx"), s.ints("status"))
        l, L = s.gains()
        if ref is None:
            ref = out + (l, L)
        else:
            for a, r in zip(out + (l, L), ref):
                assert np.array_equal(a, r)
        s.close()


def test_wave_mapping_results_do_not_depend_on_stream_groups(ilqg):
    """the same for the wave mapping (n = 16 problem): several contexts share the device's work buffer, the roll-out stream
    and — for the kernels with scratch memory — that stream's queue (on_scratch_stream); ragged group sizes, a horizon
    that lets wavefronts of the derivative kernel straddle trajectories"""
    B, N, iters = 150, 40, 4
    x0, u0 = syn_inputs(B, N)
    ref = None
    for groups in (1, 2, 3):
        s = ilqg.BatchSolver("synth16x8", 1, batch=B, n_hor=N, params=SYN_PARAMS_TIGHT, opts=dict(max_iter=iters + 1), groups=groups)
        assert s.groups() == groups
        s.init(x0, u0)
        s.iterate(iters)
        out = (s.scalar("cost"), s.scalar("lambda"), s.x(), s.u(), s.ints("alpha_idx"), s.ints("status"), s.ints("bp_calls"))
        s.close()
        if ref is None:
            ref = out
        else:
            for a, r in zip(out, ref):
                assert np.array_equal(a, r)


def test_huge_angle_goes_through_the_library_sincos(ilqg, synth, oracle_built):
    """sin/cos of the generated callbacks are straight-line code for |x| < 8e5; beyond that the step is evaluated
    a second time through the device library (the `huge` hook).  A heading angle of 1e7 rad in ONE trajectory of
    a wavefront: that trajectory matches the CPU (exact range reduction), its neighbours are untouched."""
    B, iters = 64, 3
    x0, u0 = synth.car_batch(B, first=500)
    x0 = x0.copy()
    x0[5, 2] = 1.0e7 + 0.25
    s = ilqg.BatchSolver("carparking", 0, batch=B, n_hor=500, params=ilqg.CAR_PARAMS, opts=dict(max_iter=iters))
    s.init(x0, u0)
    c0 = s.scalar("cost")
    s.iterate(iters)
    cost, x = s.scalar("cost"), s.x()
    for b in (4, 5, 6):
        d = Driver(lib_path("oracle", full_ddp=0), 500, CAR_PARAMS, dict(max_iter=iters))
        assert d.init(x0[b], u0[b]) == 1
        if b == 5:
            assert close(c0[b], d.scalars()["cost"], 1e-9)   # initial roll-out
        d.solve()
        assert close(cost[b], d.scalars()["cost"], 1e-8), (b, cost[b], d.scalars()["cost"])
        assert np.abs(x[b] - d.traj(0)[0]).max() < 1e-6 * max(1.0, np.abs(x[b]).max())
        d.close()
    # and the unfused derivative kernel takes the same path
    s2 = ilqg.BatchSolver("carparking", 0, batch=B, n_hor=500, params=ilqg.CAR_PARAMS, opts=dict(max_iter=iters, fuse_derivs=0))
    s2.init(x0, u0)
    s2.iterate(iters)
    assert np.allclose(s2.scalar("cost"), cost, rtol=1e-9, atol=0)
    s.close(); s2.close()


# ---------------------------------------------------------------------------
# edge cases: failures, exits, degenerate sizes
# ---------------------------------------------------------------------------
def test_failure_paths_are_per_trajectory(ilqg, synth):
    """NaN in one trajectory's inputs fails THAT trajectory (status 7, as iLQG_mex.c:116-118 reports a failed
    initial roll-out) and leaves its neighbours in the same wavefront untouched"""
    B, iters = 66, 3
    x0, u0 = synth.car_batch(B, first=4000)
    clean = ilqg.BatchSolver("carparking", 0, batch=B, n_hor=500, params=ilqg.CAR_PARAMS, opts=dict(max_iter=iters))
    clean.init(x0, u0)
    clean.iterate(iters)
    u_bad = u0.copy()
    u_bad[5, 100, 0] = np.nan
    x_bad = x0.copy()
    x_bad[64, 3] = np.inf
    s = ilqg.BatchSolver("carparking", 0, batch=B, n_hor=500, params=ilqg.CAR_PARAMS, opts=dict(max_iter=iters))
    s.init(x_bad, u_bad)
    st = s.ints("status")
    assert st[5] == 7 and st[64] == 7 and np.all(np.delete(st, [5, 64]) == 0)
    s.iterate(iters)
    ok = np.ones(B, dtype=bool); ok[[5, 64]] = False
    assert np.array_equal(s.scalar("cost")[ok], clean.scalar("cost")[ok])
    assert np.array_equal(s.x()[ok], clean.x()[ok])
    assert np.all(s.ints("status")[~ok] == 7) and np.all(s.success()[~ok] == 0)
    s.close(); clean.close()


@pytest.mark.parametrize("problem", ["synth16x8", "synth16x8_plain"])
@pytest.mark.parametrize("fd", [0, 1])
def test_failure_paths_are_per_trajectory_with_uniform_guards(ilqg, fd, problem):
    """the large generated file (n = 16) is compiled with wave-uniform NaN/Inf guards: when one lane's value is not
    finite every lane of the wavefront leaves the callback, and the kernel repeats the call lane by lane.  A NaN
    in one trajectory's inputs (initial roll-out) and an Inf planted in another one's state (derivatives) must fail
    exactly those two and leave every other trajectory's results bit-identical to a clean run (the repetition runs
    the same machine code as the first attempt).  `_plain`: the pair without hints, whose callbacks work on the private
    element with proxies (ilqgdev) — the repetition then writes each lane's entries out by itself (mode ALONE)."""
    B, N, iters = 70, 32, 2
    x0, u0 = syn_inputs(B, N)
    runs = []
    for poison in (False, True):
        u = u0.copy()
        if poison:
            u[5, 10, 3] = np.nan
        s = ilqg.BatchSolver(problem, fd, batch=B, n_hor=N, params=SYN_PARAMS_TIGHT, opts=dict(max_iter=iters + 1))
        s.init(x0, u)
        if poison:
            st = s.ints("status")
            assert st[5] == 7 and np.all(np.delete(st, 5) == 0)
            x = s.x()
            x[40, 7, 2] = np.inf
            s.set_x(x)
        s.iterate(iters)
        runs.append((s.ints("status"), s.scalar("cost"), s.x(), s.u(), s.ints("iterations")))
        s.close()
    clean, bad = runs
    ok = np.ones(B, dtype=bool); ok[[5, 40]] = False
    assert bad[0][5] == 7 and bad[0][40] == 6
    for a, b in zip(clean, bad):
        assert np.array_equal(a[ok], b[ok])


def test_line_search_staging_in_the_wave_mapping(ilqg):
    """n = 16 problem (one wavefront per trajectory in the backward pass, records only): one stage, two stages with kept
    or re-rolled trajectories — the same bits"""
    B, N, iters = 150, 40, 4
    x0, u0 = syn_inputs(B, N)
    ref = None
    for opts in (dict(ls_split=0), dict(ls_split=1), dict(ls_split=3), dict(ls_split=1, ls_keep=0), dict(ls_split=5, ls_keep=0)):
        # (zMin: a demanding acceptance test, so that the later step sizes are needed)
        s = ilqg.BatchSolver("synth16x8", 1, batch=B, n_hor=N, params=SYN_PARAMS_TIGHT, opts=dict(max_iter=iters + 1, zMin=0.97, **opts))
        s.init(x0, u0)
        hist = []
        for _ in range(iters):
            s.iterate(1)
            hist.append((s.ints("alpha_idx").copy(), s.ints("accepted").copy(), s.scalar("cost").copy(), s.scalar("new_cost").copy()))
        out = (hist, s.x(), s.u())
        s.close()
        if ref is None:
            ref = out
            assert np.concatenate([h[0] for h in hist]).max() >= 2  # later step sizes are needed
            continue
        for h, hr in zip(out[0], ref[0]):
            for a, r in zip(h, hr):
                assert np.array_equal(a, r), opts
        assert np.array_equal(out[1], ref[1]) and np.array_equal(out[2], ref[2]), opts


@pytest.mark.parametrize("problem,n_hor", [("synth16x8", 40), ("carparking_wave", 60)])
def test_wave_rollouts_through_lds_equal_per_lane_loads(ilqg, monkeypatch, problem, n_hor):
    """wave mapping: the roll-outs that fetch the nominal records once per step and workgroup into LDS
    (k_rollout_parts<true>, global_load_lds) against the same kernel with per-lane loads (ILQG_NO_DMA=1): the same bits,
    with ragged batches (a partly filled last workgroup) and a second stage that walks the pending list"""
    wave = problem.endswith("_wave")
    name = problem[:-5] if wave else problem
    fd = 0 if wave else 1
    B, iters = (150, 4) if not wave else (200, 5)
    if wave:
        n_hor = 500  # (the generator of the CarParking batch makes whole horizons)
        x0, u0 = load_package().synth.car_batch(B)
        params = ilqg.CAR_PARAMS
    else:
        (x0, u0), params = syn_inputs(B, n_hor), SYN_PARAMS_TIGHT
    res = []
    for no_dma in ("", "1"):
        if no_dma:
            monkeypatch.setenv("ILQG_NO_DMA", no_dma)
        else:
            monkeypatch.delenv("ILQG_NO_DMA", raising=False)
        s = ilqg.BatchSolver(name, fd, batch=B, n_hor=n_hor, params=params, opts=dict(max_iter=iters + 1, zMin=0.9),
                             strict="wave" if wave else False)
        assert s.problem.wave_mapping
        s.init(x0, u0)
        s.iterate(iters)
        res.append((s.ints("alpha_idx").copy(), s.ints("accepted").copy(), s.scalar("cost").copy(), s.x(), s.u()))
        s.close()
    monkeypatch.delenv("ILQG_NO_DMA", raising=False)
    assert res[0][0].max() >= 2  # (later step sizes are needed: the second stage ran)
    for a, b in zip(*res):
        assert np.array_equal(a, b)


@pytest.mark.parametrize("fd", [0, 1])
def test_backward_on_two_wavefronts_equals_one(ilqg, synth, fd):
    """option bw_split: the fused backward pass with the derivatives of step k-1 on a second wavefront (hand-over of the
    time-varying record entries in LDS, one barrier per step) — every bit as on one wavefront, through lambda retries
    (FULL_DDP = 1: up to 6 sweeps per pass in these iterations), a ragged last tile and a trajectory whose derivatives
    fail"""
    B, N, iters = 97, 500, 10
    x0, u0 = synth.car_batch(B, N, first=4100)
    runs = []
    for split in (0, 1):
        s = ilqg.BatchSolver("carparking", fd, batch=B, n_hor=N, params=ilqg.CAR_PARAMS, opts=dict(max_iter=iters + 2, bw_split=split), strict="exp")
        s.init(x0, u0)
        x = s.x()
        x[70, 300, 3] = np.inf
        s.set_x(x)
        snaps = []
        for it in range(iters):
            s.iterate(1)
            l, L = s.gains()
            snaps.append((l, L, s.scalar("dV0"), s.scalar("dV1"), s.scalar("lambda"), s.scalar("g_norm"), s.scalar("cost"),
                          s.ints("bp_calls"), s.ints("bp_rc"), s.ints("status"), s.x(), s.u()))
        runs.append(snaps)
        s.close()
    assert runs[0][0][9][70] == 6 and max(snap[7].max() for snap in runs[0]) >= (3 if fd else 1)  # (FULL_DDP = 0 needs no retries here)
    for a, b in zip(*runs):
        for p, q in zip(a, b):
            assert np.array_equal(p, q, equal_nan=True)


@pytest.mark.parametrize("fd", [0, 1])
def test_chunked_records_with_a_finished_trajectory(ilqg, fd, monkeypatch):
    """a work buffer that holds a fraction of the batch (records evaluated and consumed chunk by chunk, the chunks
    taking turns in the two halves of the buffer): same results as with room for everything, also when a
    trajectory that is out of the race (failed initial roll-out) sits in a slot another one uses later — the constant
    entries of the records are written for every slot, not only for the active trajectories' (regression)."""
    import gc
    B, N, iters = 70, 32, 2
    x0, u0 = syn_inputs(B, N)
    u0 = u0.copy()
    u0[5, 10, 3] = np.nan
    runs = []
    for work_gb in (None, 0.012 if fd == 0 else 0.02):
        gc.collect()  # the device's work buffer goes with its last user and is sized by the next first one
        if work_gb is None:
            monkeypatch.delenv("ILQG_WORK_GB", raising=False)
        else:
            monkeypatch.setenv("ILQG_WORK_GB", str(work_gb))
        s = ilqg.BatchSolver("synth16x8", fd, batch=B, n_hor=N, params=SYN_PARAMS_TIGHT, opts=dict(max_iter=iters + 1))
        s.timing(True)
        s.init(x0, u0)
        s.iterate(iters)
        l, L = s.gains()
        launches = s.kernel_times()["k_backward"][0]
        runs.append((s.ints("status"), s.scalar("cost"), s.x(), s.u(), l, L, launches))
        s.close()
    whole, chunked = runs
    assert whole[0][5] == 7
    assert whole[6] == iters and chunked[6] > 2 * iters, "the second run was meant to go chunk by chunk"
    ok = np.ones(B, dtype=bool); ok[5] = False
    for a, b in zip(whole[:6], chunked[:6]):
        assert np.array_equal(a[ok], b[ok])


# all inside the first 8 iterations, before free-running paths can drift apart (test_lockstep20_teacher_forced)
@pytest.mark.parametrize("opts", [dict(max_iter=0), dict(max_iter=8, alpha=[1.0], zMin=0.99, lambdaMax=3.0), dict(max_iter=6, lambdaInit=1e9),
                                  dict(max_iter=8, tolFun=0.5), dict(max_iter=8, alpha=[1.0, 0.5]), dict(max_iter=8, zMin=0.6)])
def test_exit_conditions_match_oracle(ilqg, synth, oracle_built, opts):
    """every way out of the outer loop (iLQG.c:365-378): iteration counts, return values and costs as the oracle's"""
    B = 12
    x0, u0 = synth.car_batch(B, first=6000)
    s = ilqg.BatchSolver("carparking", 0, batch=B, n_hor=500, params=ilqg.CAR_PARAMS, opts=opts)
    s.init(x0, u0)
    s.solve()
    assert s.active() == 0
    its, succ, cost = s.ints("iterations"), s.success(), s.scalar("cost")
    if "lambdaMax" in opts:
        assert np.all(s.ints("status") == 5)  # rejected steps drove lambda past lambdaMax (iLQG.c:356-360)
    for b in range(B):
        d = Driver(lib_path("oracle", full_ddp=0), 500, CAR_PARAMS, opts)
        assert d.init(x0[b], u0[b]) == 1
        rc = d.solve()
        sc = d.scalars()
        assert (int(its[b]), int(succ[b])) == (int(sc["iterations"]), rc), (opts, b, s.ints("status")[b])
        # long free-running solves drift apart (test_lockstep20_teacher_forced); the exits are what is tested
        assert close(cost[b], sc["cost"], 1e-8 if int(its[b]) <= 8 else 0.1), (opts, b)
        d.close()
    s.close()


def test_short_horizon_and_single_trajectory(ilqg, synth, oracle_built):
    """n_hor = 2 (the smallest the solver accepts: g_norm divides by n_hor - 1) and B = 1"""
    x0, u0 = synth.car_batch(1, n_hor=2, first=9)
    s = ilqg.BatchSolver("carparking", 0, batch=1, n_hor=2, params=ilqg.CAR_PARAMS, opts=dict(max_iter=5))
    s.init(x0, u0)
    s.solve()
    d = Driver(lib_path("oracle", full_ddp=0), 2, CAR_PARAMS, dict(max_iter=5))
    assert d.init(x0[0], u0[0]) == 1
    d.solve()
    assert close(s.scalar("cost")[0], d.scalars()["cost"], 1e-12) and close(s.x()[0], d.traj(0)[0], 1e-12)
    with pytest.raises(ilqg.IlqgError):
        ilqg.BatchSolver("carparking", 0, batch=1, n_hor=1, params=ilqg.CAR_PARAMS)
    with pytest.raises(ilqg.IlqgError):
        ilqg.BatchSolver("carparking", 0, batch=0, n_hor=10, params=ilqg.CAR_PARAMS)
    s.close()


def test_option_and_parameter_errors(ilqg):
    s = ilqg.BatchSolver("carparking", 0, batch=2, n_hor=10)
    with pytest.raises(ilqg.IlqgError, match="parameter must be positive"):
        s.set_option("tolFun", 0.0)
    with pytest.raises(ilqg.IlqgError, match="no such parameter"):
        s.set_option("w_pen_init", 1.0)
    with pytest.raises(ilqg.IlqgError, match="monotonically"):
        s.set_option("alpha", [1.0, 0.5, 0.5])
    with pytest.raises(ilqg.IlqgError, match="not a parameter"):
        s.set_param("nope", [1.0])
    with pytest.raises(ilqg.IlqgError, match="vector length 4"):
        s.set_param("cf", [1.0, 2.0])
    with pytest.raises(ilqg.IlqgError, match="was not set"):
        s.init(np.zeros((2, 4)), np.zeros((2, 10, 2)))  # parameters were never given
    s.close()


def test_rejected_alpha_leaves_the_step_sizes_alone(ilqg, synth):
    """a refused option value must not leak into the option set (the alpha array is only borrowed, iLQG.c:101)"""
    x0, u0 = synth.car_batch(3, 50)
    res = []
    for bad in (None, [0.5, 0.9], [2.0, 0.1]):
        s = ilqg.BatchSolver("carparking", 0, batch=3, n_hor=50, params=ilqg.CAR_PARAMS, opts=dict(ls_split=0))
        s.set_option("alpha", [1.0, 0.1])
        if bad is not None:
            with pytest.raises(ilqg.IlqgError):
                s.set_option("alpha", bad)
        s.init(x0, u0)
        s.calc_derivs(); s.back_pass(); s.line_search()
        res.append((s.scalar("alpha_cost")[:, :2].copy(), s.ints("alpha_idx").copy()))
        s.close()
    for r in res[1:]:
        assert np.array_equal(r[0], res[0][0]) and np.array_equal(r[1], res[0][1])


@pytest.mark.parametrize("problem,fd", [("carparking", 0), ("carparking", 1), ("hxtest", 1)])
def test_products_without_the_structural_zeros_equal_the_dense_ones(ilqg, synth, problem, fd):
    """Lane mapping, fused sweep: the product build leaves the terms of matMult.c's products whose record factor is
    identically 0 out (ILQG_STRUCTURAL_ZERO of the generated header; ilqg_device.hpp NoZeros), the FMA-free twin multiplies
    them out as the reference does.  With finite inputs the two differ by FMA contraction alone: gains, expected changes
    and gradient norm of a sweep at the single-pass bar (1e-10), return codes equal — over a batch, for three consecutive
    teacher-forced iterations (the twin's trajectory is handed to the product build before each sweep)."""
    if problem == "carparking":
        B, N, params = 192, 500, ilqg.CAR_PARAMS
        x0, u0 = synth.car_batch(B, N)
    else:
        B, N, params = 96, HX_N, HX_PARAMS
        x0, u0 = hx_inputs(B)
    mk = lambda strict: ilqg.BatchSolver(problem, fd, batch=B, n_hor=N, params=params, opts=dict(max_iter=8), strict=strict)
    a, b = mk(True), mk(False)
    a.init(x0, u0)
    b.init(x0, u0)
    for it in range(3):
        if it:
            b.set_x(a.x())
            b.set_u(a.u())
            for k in ("cost", "lambda", "dlambda"):
                b.set_scalar(k, a.scalar(k))
        a.back_pass(fused=True)
        b.back_pass(fused=True)
        la, La = a.gains()
        lb, Lb = b.gains()
        assert np.array_equal(a.ints("bp_rc"), b.ints("bp_rc")) and np.array_equal(a.ints("bp_calls"), b.ints("bp_calls"))
        # (the feed-forward term is the box QP's solution: once inputs run on their limits — the later iterations — the
        # iteration ends on a relative improvement of 1e-8 (boxQP.c:85), a last-bit difference of the two builds'
        # contraction may end it one iteration apart: 1e-6 there, as between two CPU builds of the reference)
        ltol = TOL if it == 0 else 1e-6
        assert close(lb, la, ltol) and close(Lb, La), (it, worst(lb, la), worst(Lb, La))
        for k in ("dV0", "dV1", "g_norm", "lambda"):
            assert close(b.scalar(k), a.scalar(k), ltol), (it, k, worst(b.scalar(k), a.scalar(k)))
        a.line_search()
        a.update()
    a.close()
    b.close()


def test_quad_lean_layout_equals_the_default(ilqg):
    """The quad-mapped backward step laid out for two wavefronts per SIMD (ilqg_quad.hpp ILQG_QUAD_LEAN = 63: 254
    registers, eight wavefronts per workgroup, values re-requested where they are used, the box QP's diagonal in LDS,
    one register set in the contraction) changes WHEN values are loaded and where they wait, not what is computed: the
    same product-build arithmetic, so gains, value changes, gradient norms, lambdas and sweep counts of a ragged batch
    with lambda retries — and the solves that follow — equal the default layout's bit for bit."""
    B, N, K = 75, 300, 4
    x0, u0 = syn_inputs(B, N, first=11)
    x0 = x0 * np.linspace(0.2, 3.0, B)[:, None]

    def run(variant):
        s = ilqg.BatchSolver("synth16x8", 1, batch=B, n_hor=N, params=SYN_PARAMS, opts=dict(max_iter=K + 1, lambdaInit=1e-7), strict=variant)
        s.init(x0, u0)
        out = []
        for it in range(K):
            s.iterate(1)
            l, L = s.gains()
            out.append(dict(l=l.copy(), L=L.copy(), dV0=s.scalar("dV0").copy(), dV1=s.scalar("dV1").copy(), g=s.scalar("g_norm").copy(),
                            lam=s.scalar("lambda").copy(), calls=s.ints("bp_calls").copy(), cost=s.scalar("cost").copy()))
        s.close()
        return out

    a, b = run(False), run("lean")
    assert np.concatenate([o["calls"] for o in a]).max() > 1
    for it, (p, q) in enumerate(zip(a, b)):
        for k in p:
            assert np.array_equal(p[k], q[k]), (it, k)


@pytest.mark.parametrize("problem,fd,strict", [("synth16x8", 1, False), ("synth16x8", 1, True), ("synth16x8", 0, False), ("synth16p", 0, False),
                                               ("synth16x8", 1, "lean")])  # (round 6: the layout of two wavefronts per SIMD speculates as well)
def test_speculative_retries_equal_the_sequential_sweeps(ilqg, monkeypatch, problem, fd, strict):
    """k_backward_quad with speculative retries (the default; k_wave_backward.inc SPEC): rows whose queue is used up run other
    trajectories' NEXT attempts (lambda_j replayed from the trajectory's lambda, iLQG.c:271-274) into buffers of their own,
    and the first attempt with a result whose predecessors all failed is what is written — the sequential loop's result
    (iLQG.c:261-283).  Batches much smaller than the kernel's 4 096 rows, so that every trajectory with a retry has
    helpers: gains, value changes, gradient norm, lambda, dlambda, status, sweep count and the trajectories of the
    iterations that follow equal those of ILQG_QUAD_SPEC=0 bit for bit; lambdaInit small enough for up to six sweeps."""
    from oracle.harness import SYNP_PARAMS_TIGHT
    params = SYNP_PARAMS_TIGHT if problem == "synth16p" else SYN_PARAMS
    seen = []
    for B, N, K in ((37, 40, 6), (300, 60, 5)):
        x0, u0 = syn_inputs(B, N, first=3)
        x0 = x0 * np.linspace(0.3, 2.5, B)[:, None]

        def run(spec):
            monkeypatch.setenv("ILQG_QUAD_SPEC", "1" if spec else "0")
            s = ilqg.BatchSolver(problem, fd, batch=B, n_hor=N, params=params, opts=dict(max_iter=K + 1, lambdaInit=1e-7), strict=strict)
            s.init(x0, u0)
            out = []
            for it in range(K):
                s.iterate(1)
                l, L = s.gains()
                out.append(dict(l=l.copy(), L=L.copy(), x=s.x().copy(), u=s.u().copy(), cost=s.scalar("cost").copy()))
                for k in ("dV0", "dV1", "g_norm", "lambda", "dlambda"):
                    out[-1][k] = s.scalar(k).copy()
                for k in ("status", "bp_calls", "bp_rc", "alpha_idx"):
                    out[-1][k] = s.ints(k).copy()
            s.close()
            return out

        a, b = run(False), run(True)
        for it, (p, q) in enumerate(zip(a, b)):
            for k in p:
                assert np.array_equal(p[k], q[k]), (B, it, k)
        seen.append(np.concatenate([o["bp_calls"] for o in a]))
    calls = np.concatenate(seen)
    if fd:  # (without the tensors Quu is positive definite: one sweep each, the kernel's other instantiation all the same)
        assert calls.max() >= 3 and (calls > 1).mean() > 0.1, (calls.max(), (calls > 1).mean())


@pytest.mark.parametrize("opts,what", [(dict(lambdaFactor=1.2), "long"), (dict(lambdaMax=1e-4), "short")])
def test_speculative_retries_under_other_lambda_schedules(ilqg, monkeypatch, opts, what):
    """The lambda schedule is the user's (lambdaFactor, lambdaMin, lambdaMax: setOptParam); the speculative kernel numbers a
    trajectory's sweeps 0..15.  "long": lambdaFactor = 1.2 allows more than 16 sweeps per call — the host takes
    the sequential loop then (ilqg_shim_impl.inc spec_sweeps_at_most) and nothing is lost.  "short": lambdaMax so small
    that trajectories run out of schedule (exit "no descent", iLQG.c:273-274) while rows speculate on them — status, lambda,
    dlambda, sweep counts and everything of the trajectories that go on equal ILQG_QUAD_SPEC=0 bit for bit; the gains of
    a trajectory that LEFT with "no descent" are those of partial sweeps in either path (nothing reads them) and are not
    compared."""
    B, N, K = 300, 60, 5
    x0, u0 = syn_inputs(B, N, first=3)
    x0 = x0 * np.linspace(0.3, 2.5, B)[:, None]

    def run(spec):
        monkeypatch.setenv("ILQG_QUAD_SPEC", "1" if spec else "0")
        s = ilqg.BatchSolver("synth16x8", 1, batch=B, n_hor=N, params=SYN_PARAMS, opts=dict(max_iter=K + 1, lambdaInit=1e-7, **opts))
        s.init(x0, u0)
        out = []
        for it in range(K):
            s.iterate(1)
            l, L = s.gains()
            out.append(dict(l=l.copy(), L=L.copy(), x=s.x().copy(), u=s.u().copy(), cost=s.scalar("cost").copy()))
            for k in ("dV0", "dV1", "g_norm", "lambda", "dlambda"):
                out[-1][k] = s.scalar(k).copy()
            for k in ("status", "bp_calls", "bp_rc", "alpha_idx"):
                out[-1][k] = s.ints(k).copy()
        s.close()
        return out

    a, b = run(False), run(True)
    NO_DESCENT = 4
    for it, (p, q) in enumerate(zip(a, b)):
        assert np.array_equal(p["status"], q["status"]), it
        live = p["status"] != NO_DESCENT
        for k in p:
            if k in ("l", "L"):
                assert np.array_equal(p[k][live], q[k][live]), (it, k)
            else:
                assert np.array_equal(p[k], q[k]), (it, k)
    calls = np.concatenate([o["bp_calls"] for o in a])
    status = a[-1]["status"]
    if what == "short":
        assert (status == NO_DESCENT).sum() >= 3 and (status != NO_DESCENT).sum() >= 3, np.bincount(status)
    else:
        assert calls.max() >= 4, calls.max()


def test_private_element_with_proxies_changes_nothing(ilqg):
    """The hint-free n = 16 pair's callbacks work on a private element whose derivative arrays are proxies (an assignment goes
    into a ring in LDS, runs of entries are written out by the wavefront: ilqg_kernels.hip ilqgdev, tools/gen_record_dev.py)
    — against the same pair built with -DILQG_DEV_ELEMENT=0 (the callbacks store into the record in HBM entry by entry, as
    every such pair did before round 6): the derivative records the host reads back, and four lock-step iterations with
    lambda retries, bit for bit.  The generated arithmetic is the same text in both; this pins the plumbing — slot
    addresses, run ends, write-outs, constants, limits, a ragged batch with lanes that copy."""
    B, N, K = 37, 45, 4
    x0, u0 = syn_inputs(B, N, first=9)
    x0 = x0 * np.linspace(0.4, 2.2, B)[:, None]
    out = []
    for build in (False, "direct"):
        s = ilqg.BatchSolver("synth16x8_plain", 1, batch=B, n_hor=N, params=SYN_PARAMS, opts=dict(max_iter=K + 1, lambdaInit=1e-7), strict=build)
        s.init(x0, u0)
        s.calc_derivs()
        rec, fin = s.derivs()
        res = [rec.copy(), fin.copy()]
        for it in range(K):
            s.iterate(1)
            l, L = s.gains()
            res += [l.copy(), L.copy(), s.x().copy(), s.u().copy(), s.scalar("cost").copy(), s.scalar("lambda").copy(), s.ints("bp_calls").copy(),
                    s.ints("alpha_idx").copy()]
        s.close()
        out.append(res)
    assert np.concatenate([r for r in out[0][8::8]]).max() > 1  # lambda retries happen
    for i, (a, b) in enumerate(zip(*out)):
        assert np.array_equal(a, b), i


def test_stored_tensors_in_the_quad_mapping_equal_the_row_mapping(ilqg, monkeypatch):
    """The hint-free n = 16 pair (stored tensors; its limitsU stores only zeros as the limits' gradients, which the build reads
    off the function file: tools/gen_record_dev.py limits_state_free) through k_backward_quad with the tensors read from the
    records (ILQG_QUAD_STORED=1, ilqg_quad.hpp: 16-byte pieces a few slices ahead) against the row-mapped default: the first
    iteration's sweeps (lambda retries included) term by term to rounding — the product build's quad step leaves the
    symmetric half sums out, DESIGN 2.2 — and three more iterations to the same accepted step sizes and costs."""
    B, N, K = 23, 40, 4
    x0, u0 = syn_inputs(B, N, first=5)

    def run(quad):
        monkeypatch.setenv("ILQG_QUAD_STORED", "1" if quad else "0")
        s = ilqg.BatchSolver("synth16x8_plain", 1, batch=B, n_hor=N, params=SYN_PARAMS, opts=dict(max_iter=K + 1, lambdaInit=1e-7))
        s.init(x0, u0)
        out = []
        for it in range(K):
            s.iterate(1)
            l, L = s.gains()
            out.append(dict(l=l.copy(), L=L.copy(), x=s.x().copy(), cost=s.scalar("cost").copy(), dV0=s.scalar("dV0").copy(),
                            calls=s.ints("bp_calls").copy(), alpha=s.ints("alpha_idx").copy()))
        s.close()
        return out

    a, b = run(False), run(True)
    assert np.concatenate([o["calls"] for o in a]).max() > 1
    for k in a[0]:
        if k in ("calls", "alpha"):
            assert np.array_equal(a[0][k], b[0][k]), k
        else:
            assert np.allclose(a[0][k], b[0][k], rtol=1e-8, atol=1e-10), (k, float(np.abs(a[0][k] - b[0][k]).max()))
    for it in range(1, K):
        assert np.array_equal(a[it]["alpha"], b[it]["alpha"]), it
        assert np.allclose(a[it]["cost"], b[it]["cost"], rtol=1e-7), it


@pytest.mark.parametrize("strict", [True, False])
def test_factored_records_with_state_dependent_limits(ilqg, oracle_built, strict):
    """n > 8, FULL_DDP = 1 from the factored tensor tables, AND input limits that depend on the state (problems/defs/
    synth10hx.py): limitsU() stores the limits' signs and gradients into the element, the row-mapped factored
    backward step reads them from the record (ilqg_row.hpp, back_pass.c:186-199) — so k_derivs_wave's factored
    instantiation must work on the record itself here, not on its private element.  Five lock-step iterations of a ragged
    batch, teacher forced (before each iteration the batch gets the oracle's trajectories: an input that sits ON a limit
    which moves with the state makes the box QP's clamp decision a matter of the last bit, and a free-running pair parts
    ways there — trajectory 7 does in iteration 2), each against the oracle's next state: accepted step size and sweep count
    equal, cost and trajectory to rounding; with limits active whose gradients are not zero."""
    from oracle.harness import SYN10_PARAMS, syn10_inputs
    B, N, iters = 21, 40, 5
    x0, u0 = syn10_inputs(B, N)

    def oracle_state(b, n_it):
        d = Driver(lib_path("oracle", "synth10hx", 1), N, SYN10_PARAMS, dict(max_iter=max(n_it, 1)))
        assert d.init(x0[b], u0[b]) == 1
        if n_it:
            d.solve()
        sc, (xx, uu), tr = d.scalars(), d.traj(0), d.trace()
        d.close()
        return sc, xx, uu, tr
    states = [[oracle_state(b, it) for b in range(B)] for it in range(iters + 1)]
    s = ilqg.BatchSolver("synth10hx", 1, batch=B, n_hor=N, params=SYN10_PARAMS, opts=dict(max_iter=iters + 1), strict=strict)
    assert s.problem.wave_mapping and (s.problem.nx, s.problem.nu) == (10, 3)
    s.init(x0, u0)
    on_state_limit = 0
    for it in range(iters):
        s.set_x(np.array([states[it][b][1] for b in range(B)]))
        s.set_u(np.array([states[it][b][2] for b in range(B)]))
        s.set_scalar("cost", np.array([states[it][b][0]["cost"] for b in range(B)]))
        s.iterate(1)
        cost, lam, aidx, calls, x, u = s.scalar("cost"), s.scalar("lambda"), s.ints("alpha_idx"), s.ints("bp_calls"), s.x(), s.u()
        for b in range(B):
            sc, xr, ur, tr = states[it + 1][b]
            assert aidx[b] == tr["alpha_idx"][it] and calls[b] == tr["bp_calls"][it], (it, b)
            assert close(lam[b], sc["lambda"], 1e-12), (it, b)
            assert close(cost[b], sc["cost"], 1e-9), (it, b, cost[b], sc["cost"])
            assert np.abs(x[b] - xr).max() < 1e-7 and np.abs(u[b] - ur).max() < 1e-7, (it, b)
            # inputs sitting on a limit that moves with the state: u0 on lim + x1 / 2, u2 on -(lim + x0^2 / 5)
            on_state_limit += int(np.sum(np.abs(ur[:, 0] - (0.3 + xr[:-1, 1] / 2)) < 1e-12) + np.sum(np.abs(ur[:, 2] + (0.3 + xr[:-1, 0] ** 2 / 5)) < 1e-12))
    s.close()
    assert on_state_limit > 100, on_state_limit
