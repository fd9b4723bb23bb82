"""TEST INFRASTRUCTURE — one generator of backward sweeps under the reference's second regularisation (regType 2,
back_pass.c:136-155: lambda fu'fu onto Quu and lambda fx'fu onto Qxu, through the reference's literal index expressions,
SURVEY Appendix B-1) for every device restatement of it: back_step (lane mapping, stored and fused sweeps),
back_step_row (row mapping) and back_step_wave (one output element per lane).  tests/test_regtype2_cases_recipe.py pins
the generator to the reference build and to tests/golden/regtype2.npz (no GPU); tests/test_gpu_regtype2.py uses it.

A case is (problem, FULL_DDP).  Its start is
    roll   the initial roll-out of the problem's seeded inputs (every FULL_DDP = 0 case; hxtest, almix, brachi_hli)
    it3    the nominal trajectory after 3 regType-1 iterations of the CPU driver from those inputs
           (carparking, synth16x8, synth10hx at FULL_DDP = 1: from their roll-outs the reference abandons every sweep or
           completes only at one end of the grid)
— installed as the roll-out of the start's controls (see _driver_at) — and at every lambda of its grid ONE back_pass()
follows calc_derivs() on a fresh driver whose gains were filled with NaN:
the steps whose L came back finite are the steps the sweep completed (back_pass.c:175 writes L behind the box QP; l is
written in front of it, as the warm start, and says nothing).

TABLE below is what the reference gives, case by case: (problem, fd, start, n_hor, lambda, rc, completed steps, bar).
`bar` is what the product (FMA-contracting) build is held to: None = the suite's single-pass tolerance (1e-10 relative to
max(1, |ref|), `close` of tests/test_gpu_parity.py); a number = 10 times what FMA contraction does to the reference's own
sources on that line (fma_distance), where the product build misses the tolerance and its FMA-free twin is exact.  The
FMA-free builds are held bit for bit at every line.  The
recipe test asserts the table line by line, and the three conditions every (problem, fd) has to meet:
    - at least two completed sweeps at lambda > 0;
    - carparking / synth16x8 / synth10hx at FULL_DDP = 1: at least one sweep abandoned behind at least one completed step;
    - at every completed lambda > 0 the gains differ from the regType-1 gains of the same lambda by at least 1e4 bars
      (worst element, relative to max(1, |ref|)): a kernel that ignored regType cannot pass.
"""
import ctypes as C
import os

import numpy as np

from oracle.harness import (ALMIX_N, CAR_PARAMS, CAR_X0, HX_N, HX_PARAMS, SYN10_PARAMS, SYN_PARAMS_TIGHT, Driver, almix_case, brachi_hli_case,
                            hx_inputs, lib_path, syn10_inputs, syn_inputs)

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "regtype2.npz")
TOL = 1e-10  # the suite's single-pass tolerance
CAR_N = 30   # the shortest of 20, 30, 40, 60, 100 at which all three conditions hold for CarParking (both FULL_DDP)
IT3 = (("carparking", 1), ("synth16x8", 1), ("synth10hx", 1))
PROBLEMS = ("carparking", "hxtest", "synth16x8", "synth10hx", "almix", "brachi_hli")

# (problem, fd, start, n_hor, lambda, reference rc, completed steps, bar of the product build)
TABLE = [
    ("carparking", 0, "roll", 30, 0.0, 0, 30, None),
    ("carparking", 0, "roll", 30, 0.001, 0, 30, None),
    ("carparking", 0, "roll", 30, 1.0, 0, 30, None),
    ("carparking", 0, "roll", 30, 1000.0, 0, 30, None),
    ("carparking", 1, "it3", 30, 0.0, 1, 26, None),
    ("carparking", 1, "it3", 30, 1.0, 1, 26, None),
    ("carparking", 1, "it3", 30, 30.0, 1, 26, None),
    ("carparking", 1, "it3", 30, 1000.0, 0, 30, None),
    ("carparking", 1, "it3", 30, 10000.0, 0, 30, None),
    ("hxtest", 0, "roll", 120, 0.0, 0, 120, None),
    ("hxtest", 0, "roll", 120, 0.001, 0, 120, None),
    ("hxtest", 0, "roll", 120, 1.0, 0, 120, None),
    ("hxtest", 0, "roll", 120, 1000.0, 0, 120, None),
    ("hxtest", 1, "roll", 120, 0.0, 0, 120, None),
    ("hxtest", 1, "roll", 120, 0.001, 0, 120, None),
    ("hxtest", 1, "roll", 120, 1.0, 0, 120, None),
    ("hxtest", 1, "roll", 120, 1000.0, 0, 120, None),
    ("synth16x8", 0, "roll", 32, 0.0, 0, 32, None),
    ("synth16x8", 0, "roll", 32, 0.001, 0, 32, None),
    ("synth16x8", 0, "roll", 32, 1.0, 0, 32, None),
    ("synth16x8", 0, "roll", 32, 1000.0, 0, 32, None),
    ("synth16x8", 1, "it3", 32, 0.0, 1, 6, None),
    ("synth16x8", 1, "it3", 32, 1.0, 1, 9, None),
    ("synth16x8", 1, "it3", 32, 1000.0, 1, 27, None),
    ("synth16x8", 1, "it3", 32, 10000.0, 0, 32, None),
    ("synth16x8", 1, "it3", 32, 100000.0, 0, 32, None),
    ("synth10hx", 0, "roll", 32, 0.0, 0, 32, None),
    ("synth10hx", 0, "roll", 32, 0.001, 0, 32, None),
    ("synth10hx", 0, "roll", 32, 1.0, 0, 32, None),
    ("synth10hx", 0, "roll", 32, 1000.0, 0, 32, None),
    ("synth10hx", 1, "it3", 32, 0.0, 1, 20, None),
    ("synth10hx", 1, "it3", 32, 1.0, 1, 20, None),
    ("synth10hx", 1, "it3", 32, 30.0, 0, 32, None),
    ("synth10hx", 1, "it3", 32, 1000.0, 0, 32, None),
    # (the reference's own sources built with FMA contraction and nothing else changed, oracle/_ref/libref_synth10hx_fd1_contract.so,
    # leave the FMA-free build's gains by 1.27e-10 on this line, sweeping over the same records: 10 times that.  The product
    # build is 1.97e-10 away from those records and 4.1e-10 from the device's own.)
    ("synth10hx", 1, "it3", 32, 10000.0, 0, 32, 1.3e-9),
    ("almix", 0, "roll", 80, 0.0, 0, 80, None),
    ("almix", 0, "roll", 80, 0.001, 0, 80, None),
    ("almix", 0, "roll", 80, 1.0, 0, 80, None),
    ("almix", 0, "roll", 80, 1000.0, 0, 80, None),
    ("almix", 1, "roll", 80, 0.0, 0, 80, None),
    ("almix", 1, "roll", 80, 0.001, 0, 80, None),
    ("almix", 1, "roll", 80, 1.0, 0, 80, None),
    ("almix", 1, "roll", 80, 1000.0, 0, 80, None),
    ("brachi_hli", 0, "roll", 60, 0.0, 0, 60, None),
    ("brachi_hli", 0, "roll", 60, 0.001, 0, 60, None),
    ("brachi_hli", 0, "roll", 60, 1.0, 0, 60, None),
    ("brachi_hli", 0, "roll", 60, 1000.0, 0, 60, None),
    ("brachi_hli", 1, "roll", 60, 0.0, 0, 60, None),
    ("brachi_hli", 1, "roll", 60, 0.001, 0, 60, None),
    ("brachi_hli", 1, "roll", 60, 1.0, 0, 60, None),
    ("brachi_hli", 1, "roll", 60, 1000.0, 0, 60, None),
]


def table(problem=None, fd=None):
    return [t for t in TABLE if (problem is None or t[0] == problem) and (fd is None or t[1] == fd)]


def lambdas(problem, fd):
    return [t[4] for t in table(problem, fd)]


def inputs(problem, first=0):
    """(n_hor, params, opts, x0, u0) of one start of `problem`; first = 0 is the start of TABLE, the others are the
    batch tests' further starts"""
    if problem == "carparking":
        rng = np.random.default_rng(20261019 + first)
        x0 = np.array(CAR_X0) + (0.0 if first == 0 else 1.0) * np.array([0.5, 0.5, 0.5, 0.2]) * rng.uniform(-1, 1, 4)
        return CAR_N, CAR_PARAMS, {}, x0, 0.1 * rng.standard_normal((CAR_N, 2))
    if problem == "hxtest":
        x0, u0 = hx_inputs(1, first)
        return HX_N, HX_PARAMS, {}, x0[0], u0[0]
    if problem == "synth16x8":
        x0, u0 = syn_inputs(1, 32, first=7 + first)
        return 32, SYN_PARAMS_TIGHT, {}, x0[0], u0[0]
    if problem == "synth10hx":
        x0, u0 = syn10_inputs(1, 32, seed=7 + first)
        return 32, SYN10_PARAMS, {}, x0[0], u0[0]
    if problem == "almix":
        params, opts, x0, u0 = almix_case(None, seed=3 + first)
        return ALMIX_N, params, {k: v for k, v in opts.items() if k != "max_iter"}, x0, u0
    if problem == "brachi_hli":
        params, opts, x0, u0 = brachi_hli_case(60)
        return 60, params, {k: v for k, v in opts.items() if k != "max_iter"}, x0, u0 * (1.0 + 0.05 * first)
    raise ValueError(problem)


_starts = {}


def start(problem, fd, first=0, kind="oracle"):
    """dict(n_hor, params, opts, x0, u, kind 'roll' | 'it3', x, cost, rec, fin): the nominal trajectory the sweeps start from
    — init(x0, u) installs it — and its derivative records, from the driver build `kind`; computed once per process"""
    key = (problem, fd, first, kind)
    if key in _starts:
        return _starts[key]
    n, params, opts, x0, u0 = inputs(problem, first)
    lib = lib_path(kind, problem, fd)
    which = "it3" if (problem, fd) in IT3 else "roll"
    u = u0
    if which == "it3":
        d = Driver(lib, n, params, dict(opts, max_iter=3))
        assert d.init(x0, u0) == 1
        d.solve()
        x, u = d.traj(0)
        cost = d.scalars()["cost"]
        d.close()
    d = _driver_at(lib, n, params, opts, x0, u, 2)
    if which == "it3":  # the roll-out of the solve's controls IS the solve's trajectory
        assert np.array_equal(d.traj(0)[0], x) and d.scalars()["cost"] == cost
    x, cost = d.traj(0)[0], d.scalars()["cost"]
    rec, fin = d.derivs()
    d.close()
    _starts[key] = dict(n_hor=n, params=params, opts=opts, x0=x0, u=u, kind=which, x=x, cost=cost, rec=rec, fin=fin)
    return _starts[key]


def _driver_at(lib, n, params, opts, x0, u, reg_type):
    """a fresh driver whose nominal trajectory is the roll-out of the controls u from x0, derivatives evaluated, lambda = 1.
    (Not set_state() in front of calc_derivs(): the generated forward_pass leaves auxiliary terms in the trajectory that
    calc_derivs reads, so records taken behind set_state belong to the roll-out before it, not to the state put in — off by
    3e-4 for CarParking and 5e-2 for the n = 16 problem three iterations in.  The open-loop roll-out of a solve's controls
    reproduces the solve's states bit for bit, auxiliaries included.)"""
    d = Driver(lib, n, params, dict(opts, regType=reg_type))
    assert d.init(x0, u) == 1
    assert d.calc_derivs() == 1
    return d


_sweeps = {}


def sweep(problem, fd, lam, reg_type=2, first=0, kind="oracle"):
    """dict(rc, l [N, nu], L [N, nu nx], dV [2], g_norm, done [N] of bool) of one back_pass() at lambda `lam` from
    start(problem, fd, first) in the driver build `kind`.  dV and g_norm are what the driver holds afterwards (behind an
    abandoned sweep: partial sums and the value from before; compared where rc == 0 only)"""
    key = (problem, fd, float(lam), reg_type, first, kind)
    if key in _sweeps:
        return _sweeps[key]
    s = start(problem, fd, first, kind)
    d = _driver_at(lib_path(kind, problem, fd), s["n_hor"], s["params"], s["opts"], s["x0"], s["u"], reg_type)
    l, L = d.gains()
    d.set_gains(np.full_like(l, np.nan), np.full_like(L, np.nan))
    d.set_lambda(lam)
    rc = d.back_pass()
    C.CDLL(None).fflush(None)
    l, L = d.gains()
    sc = d.scalars()
    d.close()
    done = np.all(np.isfinite(L), axis=1)
    if rc == 0:
        assert done.all() and np.all(np.isfinite(l))
    else:  # abandoned at step k: the steps behind it are complete, k and the steps in front of it untouched
        k = int(np.sum(~done)) - 1
        assert not done[:k + 1].any() and done[k + 1:].all()
    _sweeps[key] = dict(rc=rc, l=l, L=L, dV=np.array([sc["dV0"], sc["dV1"]]), g_norm=sc["g_norm"], done=done)
    return _sweeps[key]


def distance(a, b):
    """worst element of |a - b| relative to max(1, |b|): the measure of `close`"""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.max(np.abs(a - b) / np.maximum(1.0, np.abs(b))))


def fma_distance(problem, fd, lam):
    """how far the reference built with FMA contraction and nothing else changed (lib_path("ref_contract")) lands from the FMA-free reference build on one
    line: worst gain, `distance`; both sweep over the FMA-free build's records"""
    s = start(problem, fd, 0, "ref")
    ref = sweep(problem, fd, lam, 2, 0, "ref")
    d = Driver(lib_path("ref_contract", problem, fd), s["n_hor"], s["params"], dict(s["opts"], regType=2))
    assert d.init(s["x0"], s["u"]) == 1 and d.calc_derivs() == 1
    d.set_derivs(s["rec"], s["fin"])
    d.set_lambda(lam)
    assert d.back_pass() == ref["rc"] == 0
    l, L = d.gains()
    d.close()
    return max(distance(l, ref["l"]), distance(L, ref["L"]))


def golden_of(kind="ref"):
    """everything tests/golden/regtype2.npz records (tests/golden/make_goldens.py regtype2cases), from the build `kind`"""
    out = {}
    for problem, fd, which, n, lam, rc, ndone, bar in TABLE:
        s = start(problem, fd, 0, kind)
        tag = "%s_fd%d/" % (problem, fd)
        out[tag + "x"], out[tag + "u"], out[tag + "cost"] = s["x"], s["u"], np.array(s["cost"])
        r = sweep(problem, fd, lam, 2, 0, kind)
        tag += "%g/" % lam
        out[tag + "rc"], out[tag + "dV"], out[tag + "g_norm"], out[tag + "done"] = np.array(r["rc"]), r["dV"], np.array(r["g_norm"]), r["done"]
        out[tag + "l"], out[tag + "L"] = r["l"][r["done"]], r["L"][r["done"]]
    return out


# ---------------------------------------------------------------------------
# iterations: free-running solves under regType 2 (tests/test_gpu_regtype2.py test_iterations_match_the_oracle)
# ---------------------------------------------------------------------------
SOLVE_ITERS = 6
SOLVE_CANDIDATES = 40
# Free-running iterations are compared at 1e-8 of the cost.  Problems whose limits depend on the state have starts at which
# an input arrives at or leaves its limit by a margin at rounding resolution; there the REFERENCE's own costs move by
# 1e-3 ... 1e-1 when some of the initial controls are moved by one unit in the last place (hxtest start 3: 2.4e-3 at the
# fourth iteration, synth10hx start 3: 4e-2 at the second; regType 1 does the same on hxtest), and no implementation
# whose roll-outs differ from the reference's in the last bit can be held to it.  The solves therefore use the first five
# of the starts 0 .. SOLVE_CANDIDATES - 1 (hxtest has one) at which the reference's own costs move by less than SOLVE_STABLE under such
# changes (solve_sensitivity; a property of the reference alone, asserted by the recipe test):
SOLVE_STABLE = 1e-12
SOLVE_STARTS = {("carparking", 0): (0, 1, 2, 3, 4), ("hxtest", 0): (20,), ("synth16x8", 0): (1, 2, 10, 13, 17), ("synth10hx", 0): (0, 4, 6, 8, 9),
                ("synth16x8", 1): (0, 1, 2, 4, 6), ("synth10hx", 1): (0, 3, 4, 5, 6)}


def solve(problem, fd, first, u0=None, kind="oracle"):
    """(rc, scalars, trace) of an iLQG() of SOLVE_ITERS iterations under regType 2 from start `first`"""
    n, params, opts, x0, u = inputs(problem, first)
    d = Driver(lib_path(kind, problem, fd), n, params, dict(opts, regType=2, max_iter=SOLVE_ITERS))
    assert d.init(x0, u if u0 is None else u0) == 1
    rc = d.solve()
    C.CDLL(None).fflush(None)
    out = (rc, d.scalars(), d.trace())
    d.close()
    return out


def solve_sensitivity(problem, fd, first, trials=8):
    """worst relative change of any iteration's accepted cost in the reference's own solve when a random half of the
    initial controls move up by one unit in the last place (inf: the accepted step sizes or sweep counts change)"""
    u0 = inputs(problem, first)[4]
    _, _, tr0 = solve(problem, fd, first)
    rng = np.random.default_rng(1)
    worst = 0.0
    for trial in range(trials):
        up = u0.copy()
        m = rng.random(up.shape) < 0.5
        up[m] = np.nextafter(up[m], np.inf)
        _, _, tr = solve(problem, fd, first, up)
        if not (np.array_equal(tr["alpha_idx"], tr0["alpha_idx"]) and np.array_equal(tr["bp_calls"], tr0["bp_calls"])):
            return np.inf
        if len(tr0["new_cost"]):
            worst = max(worst, distance(tr["new_cost"], tr0["new_cost"]))
    return worst
