"""TEST INFRASTRUCTURE — one generator of entries into the regularisation schedule and the gradient exit of iLQG()
(iLQG.c:261-303, 317-318, 342-343, 356-360: the retry loop around back_pass(), lambda up and down with both arms of their
max / min, the snap to zero at lambdaMin, the lambdaMax exits, g_norm < tolGrad && lambda < 1e-5) for every device
restatement of that loop.  tests/test_lambda_cases_recipe.py pins it to the reference build and to
tests/golden/lambda_schedule.npz (no GPU); tests/test_gpu_lambda_branches.py uses it.

A case is (problem, FULL_DDP, start, options, entry lambda, entry dlambda).  The start is start(problem, fd, first) of
tests/regtype2_cases.py (under regType 1), the entry goes in as lambdaInit / dlambdaInit, and the expected result is what
the reference's own iLQG() returns with max_iter = 1 (run): return value, iterations, lambda at the line search and at
return, the back_pass() calls (the trace's where a line search followed, Driver.bp_calls_pending() in front of an exit),
g_norm and dV of the last sweep; its gains (sweep_of) come from one back_pass() of regtype2_cases.sweep at the lambda the
last sweep ran at, which the recipe test holds to that run's g_norm and dV bit for bit.  dlambda is a local of iLQG(): its
expected value is schedule()'s, a plain restatement of the loop that the recipe test holds to every lambda and integer the
reference reports and whose mutants (MUTANTS) it shows to be caught.

A sequence (SEQS) is the whole loop for max_iter = 1 .. K from one entry; a mixed batch (BATCHES) is a list of
(first, lambda, dlambda) per trajectory under one option set.

tolGrad = "g" stands for the g_norm of that very sweep, "g+" for the next double above it: the ties of the gradient test.
They are resolved against the build under test (resolve), so that they are exact in a product build too.

The gradient exit behind retries needs a start whose sweep fails at lambda 0 and completes below 1e-5.  CarParking at
FULL_DDP = 1 has two among its seeded starts 0 .. 129: start 46 (fails at 0, completes at lambdaMin = 1e-6, which the exit
then snaps to 0) and start 63 (fails at 0 and 1e-6, completes at 2.56e-6).
"""
import ctypes as C
import os

import numpy as np

import regtype2_cases as R
from oracle.harness import Driver, lib_path

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "lambda_schedule.npz")
ST_ACTIVE, ST_CONVERGED_GRAD, ST_CONVERGED_FUN, ST_MAX_ITER, ST_NO_DESCENT, ST_LAMBDA_MAX = 0, 1, 2, 3, 4, 5
DEFAULTS = dict(lambdaFactor=1.6, lambdaMin=1e-6, lambdaMax=1e10, tolGrad=1e-5, tolFun=1e-7)  # iLQG.c:60-68
BELOW = float(np.nextafter(1e-5, 0.0))
G = dict(tolGrad=1e30)
F2 = dict(lambdaFactor=2.0)
CAR0, CAR1, SYN1, S10 = ("carparking", 0), ("carparking", 1), ("synth16x8", 1), ("synth10hx", 1)

CASES = {}


def _case(name, pf, lam, dlam=1.0, first=0, cls=(), **opts):
    assert name not in CASES
    CASES[name] = dict(name=name, problem=pf[0], fd=pf[1], first=first, opts=opts, lam=float(lam), dlam=float(dlam), cls=tuple(cls))


# -- the first sweep completes -------------------------------------------------------------------------------------------
_case("car0_first", CAR0, 1.0, cls=["first"])
_case("car0_above_max", CAR0, 4.0, cls=["first", "entry_above_max"], lambdaMax=2.0)
_case("car1_first", CAR1, 1e-3, cls=["first"])
_case("car1_above_max", CAR1, 1e-3, cls=["first", "entry_above_max"], lambdaMax=5e-5)
_case("syn1_first", SYN1, 1.0, cls=["first"])
_case("s10_first", S10, 0.0625, cls=["first"])
_case("hx0_first", ("hxtest", 0), 1.0, cls=["first"])
_case("almix0_first", ("almix", 0), 1.0, cls=["first"])
_case("hli0_first", ("brachi_hli", 0), 1.0, cls=["first"])
# -- 1, 3, 4 and >= 6 failed sweeps, entry dlambda = 1, < 1 / lambdaFactor, > 1 ----------------------------------------------
_case("car1_f1_one", CAR1, 4e-5, 1.0, cls=["fail1", "d_one"])
_case("car1_f1_low", CAR1, 4e-5, 0.25, cls=["fail1", "d_low"])
_case("car1_f1_high", CAR1, 4e-5, 3.0, cls=["fail1", "d_high"])
_case("car1_f3_one", CAR1, 1e-5, 1.0, cls=["fail3", "d_one"])
_case("car1_f3_low", CAR1, 1e-5, 0.25, cls=["fail3", "d_low"])
_case("car1_f3_high", CAR1, 0.0, 3.0, cls=["fail3", "d_high", "entry_zero"])
_case("car1_f4_one", CAR1, 0.0, 1.0, cls=["fail4", "d_one", "entry_zero"])
_case("car1_f4_low", CAR1, 0.0, 0.25, cls=["fail4", "d_low", "entry_zero"])
_case("s10_f4_high", S10, 1e-5, 3.0, cls=["fail4", "d_high"])
_case("s10_f6_one", S10, 0.0, 1.0, cls=["fail6", "d_one", "entry_zero"])
_case("s10_f6_low", S10, 0.0, 0.25, cls=["fail6", "d_low", "entry_zero"])
_case("syn1_f6_high", SYN1, 0.0, 3.0, cls=["fail6", "d_high", "entry_zero"])
_case("syn1_f2_3", SYN1, 1 / 32, cls=["fail3", "d_one"], **F2)
_case("syn1_f2_2", SYN1, 1 / 16, cls=["fail2", "d_one"], **F2)
_case("syn1_f2_1", SYN1, 0.25, cls=["fail1", "d_one"], **F2)
_case("syn1_f2_tie_then_done", SYN1, 1 / 32, cls=["fail3", "tie_max"], lambdaMax=2.0, **F2)
# -- entry lambda 0 behind a failing sweep, a lambdaMin of its own ------------------------------------------------------------
_case("car1_zero_min", CAR1, 0.0, cls=["entry_zero", "own_min"], lambdaMin=4e-6)
_case("syn1_zero_min", SYN1, 0.0, cls=["entry_zero", "own_min"], lambdaMin=2.0 ** -10, **F2)
# -- the lambdaMax exit behind the first, a middle and a late raise; the tie is no exit ----------------------------------------
_case("syn1_max_first", SYN1, 1 / 32, cls=["max_exit", "max_first"], lambdaMax=1 / 32, **F2)
_case("syn1_max_middle", SYN1, 1 / 32, cls=["max_exit", "max_middle"], lambdaMax=0.125, **F2)
_case("syn1_max_tie", SYN1, 1 / 32, cls=["max_exit", "max_late", "tie_max"], lambdaMax=0.25, **F2)
_case("syn1_max_late", SYN1, 1 / 32, cls=["max_exit", "max_late"], lambdaMax=1.0, **F2)
_case("car1_max_late", CAR1, 1e-6, cls=["max_exit", "max_late"], lambdaMax=5e-5)
# (the same tie in the lane mapping's kernels: 2^-17 and 2^-16 fail, 2^-14 completes)
_case("car1_f2_tie_then_done", CAR1, 2.0 ** -17, cls=["fail2", "tie_max"], lambdaMax=2.0 ** -14, **F2)
_case("car1_max_tie", CAR1, 2.0 ** -17, cls=["max_exit", "max_middle", "tie_max"], lambdaMax=2.0 ** -16, **F2)
_case("s10_max_late", S10, 0.0, cls=["max_exit", "max_late", "entry_zero"], lambdaMax=1e-5)
# (the one known difference: an exhausted retry loop with lambda < 1e-5 — see KNOWN_DIFFERENCE)
_case("car1_max_below_1e-5", CAR1, 0.0, cls=["max_exit", "known_difference"], lambdaMax=2e-6)
# -- the gradient exit ---------------------------------------------------------------------------------------------------
_case("g_exit", CAR0, 5e-6, cls=["grad", "down_above_min", "d_one"], **G)
_case("g_at_min", CAR0, 1e-6, cls=["grad", "down_at_min"], **G)
_case("g_below_min", CAR0, 5e-7, cls=["grad", "down_below_min"], **G)
_case("g_zero", CAR0, 0.0, cls=["grad", "down_zero"], **G)
_case("g_tie_lambda", CAR0, 1e-5, cls=["no_grad", "tie_lambda"], **G)
_case("g_below_tie_lambda", CAR0, BELOW, cls=["grad", "below_tie_lambda"], **G)
_case("g_lambda_false", CAR0, 1.0, cls=["no_grad", "lambda_false"], **G)
_case("g_tol_false", CAR0, 5e-6, cls=["no_grad", "tol_false"])
_case("g_tie_tol", CAR0, 5e-6, cls=["no_grad", "tie_tol"], tolGrad="g")
_case("g_above_tie_tol", CAR0, 5e-6, cls=["grad", "above_tie_tol"], tolGrad="g+")
_case("g_d_high", CAR0, 5e-6, 3.0, cls=["grad", "d_high"], **G)
_case("g_d_low", CAR0, 5e-6, 0.25, cls=["grad", "d_low"], **G)
_case("hx0_g", ("hxtest", 0), 5e-6, cls=["grad"], **G)
_case("almix0_g", ("almix", 0), 5e-6, cls=["grad"], **G)
_case("hli0_g", ("brachi_hli", 0), 5e-6, cls=["grad"], **G)
_case("syn1_g", SYN1, 0.0, first=1, cls=["grad", "down_zero"], **G)
_case("s10_g", S10, 0.0, first=1, cls=["grad", "down_zero"], **G)
_case("s10_g_tie_tol", S10, 2e-6, first=1, cls=["no_grad", "tie_tol"], tolGrad="g")
_case("s10_g_above_tie_tol", S10, 2e-6, first=1, cls=["grad", "above_tie_tol"], tolGrad="g+")
# -- the gradient exit behind retries ------------------------------------------------------------------------------------
_case("g_retry_1", CAR1, 0.0, first=46, cls=["grad", "grad_retry", "down_at_min"], **G)
_case("g_retry_2", CAR1, 0.0, first=63, cls=["grad", "grad_retry", "down_above_min"], **G)

# what the recipe test requires to be present
REQUIRED = ("first", "entry_above_max", "fail1", "fail3", "fail4", "fail6", "d_one", "d_low", "d_high", "entry_zero", "own_min", "max_first",
            "max_middle", "max_late", "tie_max", "grad", "lambda_false", "tol_false", "tie_lambda", "below_tie_lambda", "tie_tol",
            "above_tie_tol", "down_above_min", "down_at_min", "down_below_min", "down_zero", "grad_retry", "known_difference")
# every (n failed sweeps, entry dlambda) pairing the issue names
REQUIRED_PAIRS = [(f, d) for f in ("fail1", "fail3", "fail4", "fail6") for d in ("d_one", "d_low", "d_high")]
# The reference evaluates the gradient test behind an exhausted retry loop too, against the g_norm of the pass before
# (0 on entry): with lambdaMax < 1e-5 it lowers lambda once before it returns 0.  The device's back_status returns
# NO_DESCENT first.  Return value, iterations and sweeps agree; lambda and dlambda do not and are not compared.
KNOWN_DIFFERENCE = "car1_max_below_1e-5"

# sequences through the whole loop: name -> (problem, fd, first, options, entry lambda, entry dlambda, K)
REJECT = dict(alpha=[1.0], zMin=0.999999)
SEQS = {
    # accepted steps bring lambda under lambdaMin and to 0; there CarParking's sweeps complete and the solve ends in the
    # gradient exit at lambda = 0, while the n = 16 problem's sweep at 0 fails and the schedule restarts from lambdaMin
    "acc_to_zero": ("carparking", 1, 0, dict(lambdaMin=2e-4), 1e-3, 1.0, 7),
    "acc_to_zero_syn": ("synth16x8", 1, 0, dict(lambdaMin=0.75), 1.0, 1.0, 5),
    # rejected steps raise lambda from 0 through lambdaMin and both arms of both max up to the lambdaMax exit
    "rej_from_zero": ("carparking", 0, 0, dict(REJECT, lambdaMax=1e-4), 0.0, 0.25, 6),
    # ... with powers of two: the raise onto lambdaMax itself is no exit
    "rej_tie": ("carparking", 0, 0, dict(REJECT, lambdaFactor=2.0, lambdaMin=2.0 ** -30, lambdaMax=2.0 ** -10), 2.0 ** -20, 1.0, 6),
    "rej_syn": ("synth16x8", 1, 0, dict(REJECT, lambdaFactor=2.0, lambdaMax=64.0), 1.0, 1.0, 5),
}

# mixed batches: name -> (problem, fd, options, [(first, lambda, dlambda), ...]): 1-sweep lanes, lanes of 2 to >= 5 sweeps, a
# no-descent lane and a gradient-exit lane side by side (the recipe test asserts it)
_CAR_MIX = [(0, 1e-3, 1.0), (0, 4e-5, 1.0), (0, 2e-5, 1.0), (0, 1e-5, 0.25), (0, 0.0, 1.0), (4, 0.0, 1.0), (25, 0.0, 1.0), (46, 0.0, 1.0),
            (63, 0.0, 1.0), (0, 1e-5, 100.0), (94, 0.0, 1.0), (47, 5e-6, 3.0), (0, 0.0, 3.0)]
_SYN_MIX = [(0, 1.0, 1.0), (0, 0.25, 1.0), (0, 1 / 16, 1.0), (0, 1 / 32, 1.0), (0, 0.0, 1.0), (1, 0.0, 1.0), (0, 1 / 32, 64.0), (2, 0.0, 3.0),
            (4, 2e-6, 0.25), (0, 1 / 32, 128.0)]
BATCHES = {
    "car1": ("carparking", 1, dict(G, lambdaMax=1e-3), _CAR_MIX),
    "syn1": ("synth16x8", 1, dict(G, lambdaFactor=2.0, lambdaMax=4.0), _SYN_MIX),
    "s10": ("synth10hx", 1, dict(G, lambdaMax=0.5), [(0, 0.0625, 1.0), (0, 1e-3, 3.0), (0, 1e-3, 1.0), (0, 0.0, 1.0), (1, 0.0, 1.0), (0, 1e-3, 300.0), (5, 0.0, 1.0), (0, 1e-3, 400.0)]),
}


def batch_entries(name, B):
    """B entries of batch `name`: its list repeated"""
    lst = BATCHES[name][3]
    return [lst[b % len(lst)] for b in range(B)]


# ---------------------------------------------------------------------------
# the reference's own iLQG()
# ---------------------------------------------------------------------------
def resolve(opts, g_norm):
    """the options with tolGrad "g" / "g+" replaced by g_norm and the next double above it"""
    o = dict(opts)
    if o.get("tolGrad") == "g":
        o["tolGrad"] = float(g_norm)
    elif o.get("tolGrad") == "g+":
        o["tolGrad"] = float(np.nextafter(g_norm, np.inf))
    return o


def entry_g_norm(problem, fd, first, lam, kind="oracle"):
    """g_norm of the sweep at the entry lambda in the CPU build `kind` (the ties of the gradient test)"""
    r = R.sweep(problem, fd, lam, 1, first, kind)
    assert r["rc"] == 0
    return r["g_norm"]


_runs = {}


def run(problem, fd, first, opts, lam, dlam, K=1, kind="oracle"):
    """the reference's iLQG() (build `kind`) with max_iter = K from start(problem, fd, first), entered at (lam, dlam)"""
    if opts.get("tolGrad") in ("g", "g+"):
        opts = resolve(opts, entry_g_norm(problem, fd, first, lam, kind))
    key = (problem, fd, first, repr(sorted(opts.items())), float(lam), float(dlam), K, kind)
    if key in _runs:
        return _runs[key]
    s = R.start(problem, fd, first, kind)
    d = Driver(lib_path(kind, problem, fd), s["n_hor"], s["params"], dict(s["opts"], **opts, lambdaInit=lam, dlambdaInit=dlam, max_iter=K))
    assert d.init(s["x0"], s["u"]) == 1
    rc = d.solve()
    C.CDLL(None).fflush(None)
    sc, tr, pending = d.scalars(), d.trace(), d.bp_calls_pending()
    d.close()
    n_alpha = len(opts.get("alpha", range(8)))
    o = dict(DEFAULTS, **{k: v for k, v in opts.items() if k in DEFAULTS})
    T = len(tr["lambda"])
    iters = int(sc["iterations"])
    out = dict(rc=int(rc), iterations=iters, lam=sc["lambda"], ls_lambda=tr["lambda"], calls=tr["bp_calls"].astype(np.int32), pending=int(pending),
               accepted=(tr["alpha_idx"] <= n_alpha).astype(np.int32), ls_g_norm=tr["g_norm"], ls_dcost=tr["cost"] - tr["new_cost"],
               g_norm=sc["g_norm"], dV=np.array([sc["dV0"], sc["dV1"]]), cost=sc["cost"], opts=o, K=K)
    # how the run ended, as the device names it
    if pending:
        status = ST_CONVERGED_GRAD if rc == 1 else ST_NO_DESCENT
    elif iters == K:
        status = ST_MAX_ITER
    else:
        status = ST_CONVERGED_FUN if out["accepted"][T - 1] else ST_LAMBDA_MAX
    out["status"] = status
    # the last sweep: its lambda (in front of the exit's own change of it), whether it completed
    out["bp_rc"] = int(status == ST_NO_DESCENT)
    _runs[key] = out
    return out


def case_run(name, kind="oracle"):
    c = CASES[name]
    return run(c["problem"], c["fd"], c["first"], c["opts"], c["lam"], c["dlam"], 1, kind)


def seq_runs(name, kind="oracle"):
    """[run with max_iter = m for m = 1 .. K]: the state behind every iteration of the sequence"""
    problem, fd, first, opts, lam, dlam, K = SEQS[name]
    return [run(problem, fd, first, opts, lam, dlam, m, kind) for m in range(1, K + 1)]


def batch_runs(name, B=None, kind="oracle"):
    problem, fd, opts, lst = BATCHES[name]
    return [run(problem, fd, first, opts, lam, dlam, 1, kind) for first, lam, dlam in (lst if B is None else batch_entries(name, B))]


# ---------------------------------------------------------------------------
# the loop restated
# ---------------------------------------------------------------------------
MUTANTS = ("max_ge", "min_ge", "1e-5_le", "tol_le", "up_d_arm1", "up_d_arm2", "up_l_arm1", "up_l_arm2", "down_d_arm1", "down_d_arm2",
           "dlambda_reset", "no_down_on_grad")


class Diverged(Exception):
    """the restated loop asked the recorded run for a sweep or a search it does not have"""


class Replay:
    """the world of a recorded run: which sweeps failed, the g_norm of the completed ones, which searches were accepted"""

    def __init__(self, r):
        self.r, self.it, self.k = r, 0, 0

    def back_pass(self):
        r = self.r
        if self.it < len(r["calls"]):
            n, completes, g = int(r["calls"][self.it]), True, r["ls_g_norm"][self.it]
        else:
            n, completes, g = r["pending"], r["rc"] == 1, r["g_norm"]
        self.k += 1
        if self.k > n:
            raise Diverged
        return (False, g) if (self.k == n and completes) else (True, None)

    def line_search(self):
        j = self.it
        if j >= len(self.r["calls"]):
            raise Diverged
        self.it, self.k = j + 1, 0
        return bool(self.r["accepted"][j]), self.r["ls_dcost"][j]


def schedule(o, lam, dlam, K, world, mutant=None):
    """iLQG.c:227-378 with everything but lambda, dlambda and the exits left to `world`; o: the options of DEFAULTS.
    Returns dict(rc, iterations, lam, dlam, ls_lambda, ls_dlam, calls, pending, status, sweep_lambda: the lambda of every
    back_pass() in order)."""
    f, mn, mx, dlam0 = o["lambdaFactor"], o["lambdaMin"], o["lambdaMax"], dlam
    m = mutant

    def up(lam, dlam):  # iLQG.c:272-273, 342-343
        t = dlam * f
        dlam = t if m == "up_d_arm1" else f if m == "up_d_arm2" else (t if t > f else f)
        t = lam * dlam
        lam = t if m == "up_l_arm1" else mn if m == "up_l_arm2" else (t if t > mn else mn)
        return lam, dlam

    def down(lam, dlam):  # iLQG.c:298-299, 317-318
        a, b = dlam / f, 1.0 / f
        dlam = a if m == "down_d_arm1" else b if m == "down_d_arm2" else (a if a < b else b)
        lam = lam * dlam * (1.0 if (lam >= mn if m == "min_ge" else lam > mn) else 0.0)
        return lam, dlam

    def over(lam):
        return lam >= mx if m == "max_ge" else lam > mx

    out = dict(ls_lambda=[], ls_dlam=[], calls=[], sweep_lambda=[], pending=0, status=ST_MAX_ITER)
    g_norm, it, done = 0.0, 0, True
    while it < K:
        done, calls = False, 0
        while not done:
            calls += 1
            out["sweep_lambda"].append(lam)
            failed, g = world.back_pass()
            if failed:
                lam, dlam = up(lam, dlam0 if m == "dlambda_reset" else dlam)
                if over(lam):
                    break
            else:
                done, g_norm = True, g
        if (g_norm <= o["tolGrad"] if m == "tol_le" else g_norm < o["tolGrad"]) and (lam <= 1e-5 if m == "1e-5_le" else lam < 1e-5):
            if m != "no_down_on_grad":
                lam, dlam = down(lam, dlam)
            out["pending"], out["status"] = calls, (ST_CONVERGED_GRAD if done else ST_NO_DESCENT)
            break
        if not done:
            out["pending"], out["status"] = calls, ST_NO_DESCENT
            break
        out["ls_lambda"].append(lam)
        out["ls_dlam"].append(dlam)
        out["calls"].append(calls)
        accepted, dcost = world.line_search()
        if accepted:
            lam, dlam = down(lam, dlam)
            if dcost < o["tolFun"]:
                out["status"] = ST_CONVERGED_FUN
                break
        else:
            lam, dlam = up(lam, dlam)
            if over(lam):
                out["status"] = ST_LAMBDA_MAX
                break
        it += 1
    out.update(rc=int(done and it < K), iterations=it, lam=lam, dlam=dlam)
    return out


def restated(r, lam, dlam, mutant=None):
    """schedule() over the recorded run r, or None where the mutant's loop leaves the record"""
    try:
        return schedule(r["opts"], lam, dlam, r["K"], Replay(r), mutant)
    except Diverged:
        return None


def agrees(s, r):
    """a restated schedule reproduces every integer and lambda of the recorded run"""
    return (s is not None and s["rc"] == r["rc"] and s["iterations"] == r["iterations"] and s["lam"] == r["lam"] and s["pending"] == r["pending"]
            and s["status"] == r["status"] and s["calls"] == r["calls"].tolist() and s["ls_lambda"] == r["ls_lambda"].tolist())


def all_runs(kind="oracle"):
    """[(tag, run, entry lambda, entry dlambda)] of every case, sequence step and batch entry"""
    out = [("case/" + n, case_run(n, kind), c["lam"], c["dlam"]) for n, c in CASES.items()]
    for n, q in SEQS.items():
        out += [("seq/%s/%d" % (n, m + 1), r, q[4], q[5]) for m, r in enumerate(seq_runs(n, kind))]
    for n, b in BATCHES.items():
        out += [("batch/%s/%d" % (n, i), r, e[1], e[2]) for i, (e, r) in enumerate(zip(b[3], batch_runs(n, None, kind)))]
    return out


def expected(r, lam, dlam):
    """what a device run from the entry (lam, dlam) must hold: the run's own fields, dlambda from schedule(), and the state
    behind back_pass() alone (status_back, lam_back, dlam_back: in front of the line search, or at the exit)"""
    s = restated(r, lam, dlam)
    assert agrees(s, r)
    e = dict(r, dlam=s["dlam"], last_sweep_lambda=s["sweep_lambda"][-1])
    if len(r["calls"]):  # the first iteration reached its line search
        e.update(status_back=ST_ACTIVE, lam_back=r["ls_lambda"][0], dlam_back=s["ls_dlam"][0], calls_back=int(r["calls"][0]), bp_rc_back=0)
    else:
        e.update(status_back=r["status"], lam_back=r["lam"], dlam_back=s["dlam"], calls_back=r["pending"], bp_rc_back=r["bp_rc"])
    return e


def sweep_of(problem, fd, first, lam, kind="oracle"):
    """the gains (and dV, g_norm) of one back_pass() at lambda `lam` from the start: regtype2_cases.sweep under regType 1"""
    return R.sweep(problem, fd, lam, 1, first, kind)


GAINS_OF = ("car1_f4_one", "syn1_f2_3", "s10_f6_one", "g_exit", "hx0_first", "almix0_first", "hli0_first")  # one case per problem


def golden_of(kind="ref"):
    """everything tests/golden/lambda_schedule.npz records (tests/golden/make_goldens.py lambda), from the build `kind`"""
    out = {}
    for tag, r, lam, dlam in all_runs(kind):
        out[tag + "/int"] = np.array([r["rc"], r["iterations"], r["pending"], r["status"]] + r["calls"].tolist() + r["accepted"].tolist(), dtype=np.int32)
        out[tag + "/f"] = np.array([r["lam"], r["g_norm"], r["dV"][0], r["dV"][1], r["cost"]] + r["ls_lambda"].tolist())
    for n in GAINS_OF:
        c = CASES[n]
        e = expected(case_run(n, kind), c["lam"], c["dlam"])
        w = sweep_of(c["problem"], c["fd"], c["first"], e["last_sweep_lambda"], kind)
        out["gains/%s/l" % n], out["gains/%s/L" % n] = w["l"], w["L"]
    return out
