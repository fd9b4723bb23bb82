"""regType 2 (back_pass.c:136-155) on the device, in every backward step that restates it: back_step (lane mapping; the
stored sweep and the fused one), back_step_row (row mapping, LDS copies with padded leading dimensions) and back_step_wave
(one output element per lane) — against the reference's own sweeps on the cases of tests/regtype2_cases.py, which
tests/test_regtype2_cases_recipe.py pins to the reference build and to tests/golden/regtype2.npz.

Bars: the FMA-free builds (`strict`, `elem`) bit for bit; the product builds at the suite's single-pass tolerance
(|d| <= 1e-10 max(1, |ref|), `close`) but for one line of the table, whose bar is 10 times what FMA contraction does to
the reference itself there (regtype2_cases.TABLE).  Return codes and completed steps are always equal.  Every completed lambda > 0
line of the table lies at least 1e4 bars from the regType-1 gains of the same lambda (the recipe test), so a step that
ignored regType, or took another entry of fu, cannot pass.

Abandoned sweeps: both mappings leave the gains of the steps a sweep completed readable through gains() (the lane mapping's
stored sweep writes every step's gains to the tiled l / L arrays as it goes, k_lane_backward.inc backward_sweep; the wave
mapping writes them into the step records), so the gains of exactly the steps the reference completed are compared, and
the gains buffer is filled with NaN in front of every sweep so that nothing is left over from the sweep before."""
import os

import numpy as np
import pytest

import regtype2_cases as R
from oracle.harness import Driver, lib_path

pytestmark = pytest.mark.gpu

TOL = R.TOL


def close(a, b, tol=TOL):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return bool(np.all(np.abs(a - b) <= tol * np.maximum(1.0, np.abs(b))))


def worst(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.max(np.abs(a - b) / np.maximum(1.0, np.abs(b)))) if a.size else 0.0


@pytest.fixture(scope="module")
def ilqg():
    import __graft_entry__ as g
    g.build_for_tests()
    from ddp_generator_amd import ilqg as m
    if m.Problem("carparking", 0).device_count() < 1:
        pytest.fail("no HIP device visible: the GPU tests must run on the MI355X box")
    return m


# (library, the case it runs, FULL_DDP, build, mapping): build False = product (FMA contraction), True / "elem" = FMA-free,
# "wave" = a small problem forced into the row mapping (product build)
BUILDS = []
for _p in ("carparking", "hxtest", "almix", "brachi_hli"):
    for _fd in (0, 1):
        BUILDS += [(_p, _p, _fd, False, "lane"), (_p, _p, _fd, True, "lane")]
BUILDS += [("carparking_plain", "carparking", 0, False, "lane"), ("carparking_plain", "carparking", 1, False, "lane")]
for _p in ("synth16x8", "synth10hx"):
    for _fd in (0, 1):
        BUILDS += [(_p, _p, _fd, False, "row"), (_p, _p, _fd, True, "row")]
BUILDS += [("carparking", "carparking", 0, "wave", "row"), ("brachi_hli", "brachi_hli", 0, "wave", "row"), ("synth16x8", "synth16x8", 1, "elem", "elem")]
BUILD_IDS = ["%s-fd%d-%s" % (b[0], b[2], {False: "product", True: "strict"}.get(b[3], b[3])) for b in BUILDS]
EXACT = (True, "elem")


def solver_at(ilqg, lib, problem, fd, build, reg_type, firsts=(0,), records=True, opts=None, groups=0):
    """a BatchSolver on the starts `firsts` of the case (problem, fd): init() rolls the starts' controls out — the nominal
    trajectories of the cases, as on the CPU — and, records, the CPU driver's derivative records are put in place
    (fuse_derivs = 0: the sweeps read them)"""
    st = [R.start(problem, fd, f) for f in firsts]
    o = dict(st[0]["opts"], regType=reg_type)
    if records:
        o["fuse_derivs"] = 0
    o.update(opts or {})
    s = ilqg.BatchSolver(lib, fd, batch=len(st), n_hor=st[0]["n_hor"], params=st[0]["params"], opts=o, strict=build, groups=groups)
    s.init(np.array([t["x0"] for t in st]), np.array([t["u"] for t in st]))
    assert close(s.x(), np.array([t["x"] for t in st]), 1e-12) and close(s.scalar("cost"), np.array([t["cost"] for t in st]), 1e-12)
    if records:
        s.set_derivs(np.array([t["rec"] for t in st]), np.array([t["fin"] for t in st]))
    return s


def one_sweep(s, lam, fused=False):
    """dict(rc, l, L, dV0, dV1, g_norm, calls) [B, ...] of one sweep at lambda `lam`, the gains buffer NaN before it"""
    l, L = s.gains()
    s.set_gains(np.full_like(l, np.nan), np.full_like(L, np.nan))
    s.set_scalar("lambda", lam)
    s.set_scalar("dlambda", 1.0)
    if fused:
        s.back_pass(fused=True)
    else:
        s.back_pass(single_sweep=True)
    l, L = s.gains()
    return dict(rc=s.ints("bp_rc").copy(), l=l, L=L, dV0=s.scalar("dV0").copy(), dV1=s.scalar("dV1").copy(), g_norm=s.scalar("g_norm").copy(),
                calls=s.ints("bp_calls").copy())


def check_sweep(got, b, ref, exact, what, tol=TOL):
    """slot b of a device sweep against one reference sweep: rc always; a completed sweep in full, an abandoned one in the
    gains of exactly the steps the reference completed"""
    assert int(got["rc"][b]) == ref["rc"], (what, int(got["rc"][b]), ref["rc"])
    done = ref["done"]
    l, L = got["l"][b], got["L"][b]
    print("%s: rc %d, %d of %d steps; l off by %.3g, L by %.3g" % (what, ref["rc"], int(done.sum()), len(done), worst(l[done], ref["l"][done]),
                                                                   worst(L[done], ref["L"][done])))
    if exact:
        assert np.array_equal(l[done], ref["l"][done]) and np.array_equal(L[done], ref["L"][done]), (what, worst(l[done], ref["l"][done]), worst(L[done], ref["L"][done]))
    else:
        assert close(l[done], ref["l"][done], tol) and close(L[done], ref["L"][done], tol), (what, worst(l[done], ref["l"][done]), worst(L[done], ref["L"][done]))
    if ref["rc"] == 0:
        same = (lambda a, r: a == r) if exact else (lambda a, r: close(a, r, tol))
        assert same(got["dV0"][b], ref["dV"][0]) and same(got["dV1"][b], ref["dV"][1]), (what, got["dV0"][b], got["dV1"][b], ref["dV"])
        assert same(got["g_norm"][b], ref["g_norm"]), (what, got["g_norm"][b], ref["g_norm"])


# ---------------------------------------------------------------------------
# a, b: one sweep from the reference's records — completed and abandoned
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("lib,problem,fd,build,mapping", BUILDS, ids=BUILD_IDS)
def test_one_sweep_from_the_references_records(ilqg, oracle_built, lib, problem, fd, build, mapping):
    s = solver_at(ilqg, lib, problem, fd, build, 2)
    assert s.problem.wave_mapping == (mapping != "lane")
    seen = set()
    for _, _, _, _, lam, rc, ndone, bar in R.table(problem, fd):
        ref = R.sweep(problem, fd, lam)
        got = one_sweep(s, lam)
        check_sweep(got, 0, ref, build in EXACT, "%s fd%d %s lambda %g" % (lib, fd, build, lam), TOL if bar is None else bar)
        seen.add((lam > 0, ref["rc"]))
    assert (True, 0) in seen and (((True, 1) in seen) == ((problem, fd) in R.IT3))
    s.close()


# ---------------------------------------------------------------------------
# d: lambda = 0 — regType 2 is regType 1
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("lib,problem,fd,build,mapping", BUILDS, ids=BUILD_IDS)
def test_at_lambda_zero_both_regularisations_are_one(ilqg, monkeypatch, lib, problem, fd, build, mapping):
    """the same bits from the same backward step: where regType 1 would go to the quad mapping (the n = 16 problem), which
    restates regType 1 alone and whose product build contracts differently from the row mapping's, the quad mapping is
    switched off for both runs (ILQG_NO_QUAD), so that one kernel is compared with itself"""
    monkeypatch.setenv("ILQG_NO_QUAD", "1")
    out = []
    for reg_type in (2, 1):
        s = solver_at(ilqg, lib, problem, fd, build, reg_type)
        out.append(one_sweep(s, 0.0))
        s.close()
    a, b = out
    done = R.sweep(problem, fd, 0.0)["done"]
    assert np.array_equal(a["rc"], b["rc"]) and int(a["rc"][0]) == R.sweep(problem, fd, 0.0)["rc"]
    assert np.array_equal(a["l"][0][done], b["l"][0][done]) and np.array_equal(a["L"][0][done], b["L"][0][done])
    if a["rc"][0] == 0:
        for k in ("dV0", "dV1", "g_norm"):
            assert np.array_equal(a[k], b[k]), k


# ---------------------------------------------------------------------------
# c: from the device's own derivatives
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("problem,fd,build", [("carparking", 0, False), ("carparking", 1, False), ("carparking", 1, True), ("hxtest", 1, False),
                                              ("almix", 0, False), ("brachi_hli", 0, False)])
def test_lane_mapping_from_the_devices_own_derivatives(ilqg, oracle_built, problem, fd, build):
    """calc_derivs() and a stored sweep, and the fused sweep (derivatives inside the backward kernel: the retry loop is its
    own, so it runs at the lambdas the reference completes at — one sweep, lambda left alone), both against the reference's
    results at the single-pass tolerance"""
    s = solver_at(ilqg, problem, problem, fd, build, 2, records=False)
    n = 0
    for _, _, _, _, lam, rc, ndone, bar in R.table(problem, fd):
        ref = R.sweep(problem, fd, lam)
        s.set_ints("need_derivs", 1)
        s.calc_derivs()
        check_sweep(one_sweep(s, lam), 0, ref, False, "%s fd%d stored, lambda %g" % (problem, fd, lam))
        if rc == 0 and lam > 0:
            got = one_sweep(s, lam, fused=True)
            assert got["calls"][0] == 1 and s.scalar("lambda")[0] == lam
            check_sweep(got, 0, ref, False, "%s fd%d fused, lambda %g" % (problem, fd, lam))
            n += 1
    assert n >= 2
    s.close()


@pytest.mark.parametrize("problem,fd,build", [("synth16x8", 0, False), ("synth16x8", 1, False), ("synth16x8", 1, True), ("synth10hx", 0, False),
                                              ("synth10hx", 1, False), ("synth10hx", 1, True), ("carparking", 0, "wave")])
def test_wave_mapping_from_the_devices_own_derivatives(ilqg, oracle_built, problem, fd, build):
    """the wave mapping's derivative kernel (at FULL_DDP = 1 the records carry the factored tensors' products: the default
    fuse_derivs) and one sweep, against the reference's results at the single-pass tolerance (the line's own bar where the
    table gives it one)"""
    s = solver_at(ilqg, problem, problem, fd, build, 2, records=False)
    for _, _, _, _, lam, rc, ndone, bar in R.table(problem, fd):
        s.set_ints("need_derivs", 1)
        s.calc_derivs()
        check_sweep(one_sweep(s, lam), 0, R.sweep(problem, fd, lam), False, "%s fd%d %s own derivatives, lambda %g" % (problem, fd, build, lam),
                    TOL if bar is None else bar)
    s.close()


# ---------------------------------------------------------------------------
# e: batches — a tail wavefront, a partly filled workgroup, stream groups
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("problem,fd,build,B,lam,group_counts", [
    ("carparking", 0, True, 97, 1.0, (1, 2)), ("carparking", 1, True, 97, 1e3, (1, 2)), ("carparking", 1, False, 97, 30.0, (1,)),
    ("hxtest", 0, True, 97, 1e-3, (1,)), ("synth16x8", 1, True, 9, 1e4, (1,)), ("synth16x8", 0, False, 9, 1.0, (1,)),
    ("synth10hx", 1, True, 9, 1.0, (1,)), ("synth10hx", 0, True, 9, 1e3, (1,)),
    ("carparking", 1, True, 200, 1e3, (1, 4)), ("synth10hx", 1, True, 200, 30.0, (1, 4))])
def test_every_slot_of_a_batch_against_its_own_driver(ilqg, oracle_built, problem, fd, build, B, lam, group_counts):
    """B different starts, one lambda, every slot against a CPU driver of its own: 97 in the lane mapping (a second, partly
    filled wavefront), 9 in the wave mapping (a partly filled workgroup); and the same bits whatever the number of stream
    groups — a group is whole tiles of 64 trajectories, so 97 make two groups at most and it takes 200 (64 + 64 + 64 + 8)
    to have four"""
    firsts = tuple(range(B))
    out = []
    for groups in group_counts:
        s = solver_at(ilqg, problem, problem, fd, build, 2, firsts=firsts, groups=groups)
        assert s.groups() == groups
        out.append(one_sweep(s, lam))
        s.close()
    refs = [R.sweep(problem, fd, lam, first=b) for b in range(B)]
    for b in range(B):
        check_sweep(out[0], b, refs[b], build in EXACT, "%s fd%d slot %d lambda %g" % (problem, fd, b, lam))
    rcs = np.array([r["rc"] for r in refs])
    print("%s fd%d lambda %g: %d of %d sweeps completed" % (problem, fd, lam, int(np.sum(rcs == 0)), B))
    for other in out[1:]:
        assert np.array_equal(out[0]["rc"], other["rc"])
        for k in ("dV0", "dV1", "g_norm"):
            assert np.array_equal(out[0][k][rcs == 0], other[k][rcs == 0]), k
        for b in range(B):
            done = refs[b]["done"]
            assert np.array_equal(out[0]["l"][b][done], other["l"][b][done]) and np.array_equal(out[0]["L"][b][done], other["L"][b][done]), b


# ---------------------------------------------------------------------------
# f: the quad mapping has no regType 2 and is never taken
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("fd", [0, 1])
@pytest.mark.parametrize("build", [False, True])
def test_quad_mapping_is_not_taken(ilqg, oracle_built, monkeypatch, fd, build):
    """ilqg_quad.hpp restates regType 1 only; the host leaves the n = 16 problem to the row mapping under regType 2
    (quad_here).  kernel_times() keeps ONE entry, "k_backward", for both kernels of the wave mapping, so the launch cannot be
    told by its name: what is held is that whole backward passes (retry loop, the device's own derivatives) and the sweeps
    from the reference's records give, under regType 2, the bits they give with the quad mapping switched off (ILQG_NO_QUAD)
    and as many "k_backward" launches — while under regType 1 the same switch changes the product build's bits (the two
    mappings contract differently), so it is the regType that keeps the quad kernel out, not the switch being idle."""
    B = 9
    firsts = tuple(range(B))

    def run(reg_type):
        s = solver_at(ilqg, "synth16x8", "synth16x8", fd, build, reg_type, firsts=firsts, records=False, opts=dict(lambdaInit=1.0))
        s.timing(True)
        l, L = s.gains()
        s.set_gains(np.zeros_like(l), np.zeros_like(L))
        s.set_scalar("lambda", 1.0)
        s.set_scalar("dlambda", 1.0)
        s.back_pass(fused=True)
        l, L = s.gains()
        out = dict(l=l, L=L, rc=s.ints("bp_rc").copy(), calls=s.ints("bp_calls").copy(), lam=s.scalar("lambda").copy(), dV0=s.scalar("dV0").copy(),
                   g=s.scalar("g_norm").copy(), launches=s.kernel_times()["k_backward"][0])
        s.close()
        s = solver_at(ilqg, "synth16x8", "synth16x8", fd, build, reg_type, firsts=firsts)
        out["sweep"] = one_sweep(s, 1e4)
        s.close()
        return out

    monkeypatch.delenv("ILQG_NO_QUAD", raising=False)
    on2, on1 = run(2), run(1)
    monkeypatch.setenv("ILQG_NO_QUAD", "1")
    off2, off1 = run(2), run(1)
    assert np.any(on2["rc"] == 0)
    for k in on2:
        if k == "sweep":
            for kk in on2[k]:  # (NaN: the steps an abandoned sweep did not reach)
                assert np.array_equal(on2[k][kk], off2[k][kk], equal_nan=True), kk
        else:
            assert np.array_equal(on2[k], off2[k]), k
    for b in range(B):  # and those sweeps are the reference's
        check_sweep(on2["sweep"], b, R.sweep("synth16x8", fd, 1e4, first=b), build in EXACT, "synth16x8 fd%d slot %d" % (fd, b))
    if not build:
        assert not (np.array_equal(on1["l"], off1["l"]) and np.array_equal(on1["L"], off1["L"]))
    else:
        assert np.array_equal(on1["l"], off1["l"]) and np.array_equal(on1["L"], off1["L"])


# ---------------------------------------------------------------------------
# g: iterations
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("build", [False, True])
@pytest.mark.parametrize("problem,fd", sorted(R.SOLVE_STARTS))
def test_iterations_match_the_oracle(ilqg, oracle_built, problem, fd, build):
    """free-running solves under regType 2, max_iter = 6, from the starts of regtype2_cases.SOLVE_STARTS (those at which
    the reference's own solve does not depend on the last bit of its inputs; see there): iteration counts, return values,
    accepted step sizes and sweeps per iteration as the oracle's solve(), cost at 1e-8, lambda bit for bit in the FMA-free
    build (1e-12 in the product build: it is a product of the schedule's factors).  At FULL_DDP = 1 start 0 of the n = 16 and
    n = 10 problems has every sweep abandoned until lambda > lambdaMax, before any line search: 0 iterations, lambda about
    1.7e11 and status ILQG_ST_NO_DESCENT (4, the backward pass's way out, iLQG.c:273-275; ILQG_ST_LAMBDA_MAX, 5, is the
    rejected step's, iLQG.c:356-360).  A compacted solve equals the plain one bit for bit."""
    firsts = R.SOLVE_STARTS[(problem, fd)]
    B, iters = len(firsts), R.SOLVE_ITERS
    ins = [R.inputs(problem, f) for f in firsts]
    n, params, opts = ins[0][0], ins[0][1], dict(ins[0][2], regType=2, max_iter=iters)
    x0, u0 = np.array([i[3] for i in ins]), np.array([i[4] for i in ins])

    def device(compact, step):
        s = ilqg.BatchSolver(problem, fd, batch=B, n_hor=n, params=params, opts=dict(opts, compact=compact), strict=build)
        s.init(x0, u0)
        hist = []
        if step:
            for it in range(iters):
                live = s.ints("status") == 0
                s.iterate(1)
                hist.append((live, s.ints("alpha_idx").copy(), s.ints("bp_calls").copy()))
        else:
            s.solve()
        out = dict(iterations=s.ints("iterations").copy(), success=s.success(), status=s.ints("status").copy(), cost=s.scalar("cost").copy(),
                   lam=s.scalar("lambda").copy(), x=s.x(), u=s.u(), hist=hist)
        s.close()
        return out

    stepped, plain, compacted = device(0, True), device(0, False), device(1, False)
    for k in ("iterations", "success", "status", "cost", "lam", "x", "u"):
        assert np.array_equal(plain[k], compacted[k]), k
    for k in ("iterations", "cost", "lam", "x", "u"):  # (iteration by iteration: the same solve)
        assert np.array_equal(plain[k], stepped[k]), k
    for b, first in enumerate(firsts):
        rc, sc, tr = R.solve(problem, fd, first)
        print("%s fd%d %s start %d: oracle %d iterations rc %d lambda %g; device status %d, cost off by %.3g, lambda by %.3g" % (
            problem, fd, build, first, int(sc["iterations"]), rc, sc["lambda"], plain["status"][b], worst(plain["cost"][b], sc["cost"]),
            abs(plain["lam"][b] / sc["lambda"] - 1.0)))
        assert (int(plain["iterations"][b]), int(plain["success"][b])) == (int(sc["iterations"]), rc), first
        if fd == 1 and first == 0:
            assert int(sc["iterations"]) == 0 and len(tr["alpha_idx"]) == 0 and plain["status"][b] == 4 and plain["lam"][b] > 1e10
        for it in range(len(tr["alpha_idx"])):
            live, aidx, calls = stepped["hist"][it]
            assert live[b] and aidx[b] == tr["alpha_idx"][it] and calls[b] == tr["bp_calls"][it], (first, it, aidx[b], tr["alpha_idx"][it], calls[b], tr["bp_calls"][it])
        if build in EXACT:
            assert plain["lam"][b] == sc["lambda"], (first, plain["lam"][b], sc["lambda"])
        else:
            assert abs(plain["lam"][b] - sc["lambda"]) <= 1e-12 * sc["lambda"], (first, plain["lam"][b], sc["lambda"])
        assert close(plain["cost"][b], sc["cost"], 1e-8), (first, plain["cost"][b], sc["cost"])


# ---------------------------------------------------------------------------
# h: the drop-in boundary — tOptSet.regType = 2 through the product's back_pass() / line_search()
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("problem,fd", [("carparking", 0), ("synth16x8", 0)])
def test_dropin_stage_under_regtype2(ilqg, oracle_built, problem, fd):
    """the reference-style driver linked against the product's back_pass() / line_search() (tests/test_gpu_dropin.py), with
    regType = 2 in its tOptSet: one iteration's stages from the initial roll-out against the oracle, at that file's
    tolerance — and the gains are regType 2's, not regType 1's"""
    from test_gpu_dropin import stages
    n, params, opts, x0, u0 = R.inputs(problem)
    hip = os.path.join(os.path.dirname(lib_path("oracle")), "libdrv_%s_fd%d_hip.so" % (problem, fd))
    assert os.path.exists(hip), hip
    ref = Driver(lib_path("oracle", problem, fd), n, params, dict(opts, regType=2))
    dev = Driver(hip, n, params, dict(opts, regType=2))
    assert ref.init(x0, u0) == 1 and dev.init(x0, u0) == 1
    assert ref.scalars()["lambda"] == 1.0  # (lambdaInit: the lambda = 1 line of the table)
    stages(ref, dev, 0)
    want = R.sweep(problem, fd, 1.0)
    l, L = dev.gains()
    assert close(l, want["l"]) and close(L, want["L"]), (worst(l, want["l"]), worst(L, want["L"]))
    ref.close()
    dev.close()
