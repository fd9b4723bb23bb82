"""The device's regularisation schedule and gradient exit on each branch: the cases of tests/lambda_cases.py (pinned to the
reference's own iLQG() by tests/test_lambda_cases_recipe.py, no GPU) through every restatement of the loop iLQG.c:261-303 —
k_backward<0> (stored records) and <2> (fused) of the lane mapping, their rows twins, k_backward_split, the row mapping, the
quad kernel with and without speculative retries, the `_lean` and `_elem` libraries — with back_status, k_update and the
drop-in host loop behind them.

A single case runs four ways from init(): set_scalar("lambda" / "dlambda") and back_pass() on the CPU driver's derivative
records ("records"), on calc_derivs() ("stored"), back_pass(fused=True) ("fused"); and iterate(1) under max_iter = 1 with
the entry in lambdaInit / dlambdaInit, as the reference has it, fuse_derivs 1 and 0.
Held in every build: status, success(), iterations, bp_calls, bp_rc, lambda and dlambda, exactly (the rules contain no sum
to contract).  g_norm, dV and the gains of the last sweep, where it completed: bit for bit in the FMA-free builds where the
sweep's inputs are the reference's — always on "records"; on the device's own derivatives where derivs() returns the
reference's records bit for bit (brachi_hli; elsewhere the device's roll-out differs from the host's in the last place, and
the FMA-free builds were seen 2.1e-15 away at most) — and at the suite's single-pass bar (1e-10 relative to max(1, |ref|))
everywhere else, the worst deviation printed (2.7e-15 seen).  The g_norm == tolGrad tie takes tolGrad from a first device
run of the same sweep in the same build.  A gradient-exit lane
keeps x, u and cost, gets no history entry and has its lambda lowered once; a no-descent lane keeps its iteration count.
One case is the known difference (lambda_cases.KNOWN_DIFFERENCE): its lambda and dlambda are not compared."""
import os
from collections import namedtuple

import numpy as np
import pytest

import lambda_cases as LC
import regtype2_cases as R
from oracle.harness import Driver, lib_path

pytestmark = pytest.mark.gpu
TOL = 1e-10
EXACT = (True, "elem", "exp_strict")
NEVER = 1e-300  # a tolGrad no g_norm is below


@pytest.fixture(scope="module")
def ilqg():
    import __graft_entry__ as g
    g.build_for_tests()
    from ddp_generator_amd import ilqg as m
    if m.Problem("carparking", 0).device_count() < 1:
        pytest.fail("no HIP device visible: the GPU tests must run on the MI355X box")
    return m


def worst(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.max(np.abs(a - b) / np.maximum(1.0, np.abs(b)))) if a.size else 0.0


# a restatement of the loop: library build, environment switches, options, rows twin
Variant = namedtuple("Variant", "id problem fd build env opts rows")
VARIANTS = []
for _p, _fd in (("carparking", 0), ("carparking", 1), ("hxtest", 0), ("almix", 0), ("brachi_hli", 0), ("synth10hx", 1)):
    VARIANTS += [Variant("%s-fd%d-product" % (_p, _fd), _p, _fd, False, {}, {}, None), Variant("%s-fd%d-strict" % (_p, _fd), _p, _fd, True, {}, {}, None)]
VARIANTS += [Variant("carparking-fd%d-rows" % _fd, "carparking", _fd, _b, {}, {}, "car") for _fd, _b in ((0, True), (1, False))]
VARIANTS += [Variant("almix-fd0-rows", "almix", 0, True, {}, {}, "almix")]
VARIANTS += [Variant("carparking-fd0-split", "carparking", 0, "exp_strict", {}, dict(bw_split=1), None),
             Variant("carparking-fd1-split", "carparking", 1, "exp", {}, dict(bw_split=1), None)]
VARIANTS += [Variant("carparking-fd0-wave", "carparking", 0, "wave", {}, {}, None), Variant("brachi_hli-fd0-wave", "brachi_hli", 0, "wave", {}, {}, None)]
for _b, _n in ((False, "product"), (True, "strict")):
    VARIANTS += [Variant("synth16x8-fd1-%s-quad-spec" % _n, "synth16x8", 1, _b, {}, {}, None),
                 Variant("synth16x8-fd1-%s-quad-nospec" % _n, "synth16x8", 1, _b, dict(ILQG_QUAD_SPEC="0"), {}, None),
                 Variant("synth16x8-fd1-%s-row" % _n, "synth16x8", 1, _b, dict(ILQG_NO_QUAD="1"), {}, None)]
VARIANTS += [Variant("synth16x8-fd1-lean", "synth16x8", 1, "lean", {}, {}, None), Variant("synth16x8-fd1-elem", "synth16x8", 1, "elem", {}, {}, None)]
IDS = [v.id for v in VARIANTS]
SWITCHES = ("ILQG_QUAD_SPEC", "ILQG_NO_QUAD")


def transient_only(v):
    """The quad kernel sweeps records that are made and consumed in one call (fused sweeps, iterate under fuse_derivs = 1); stored
    records go to the row mapping whatever the switches say (ILQG_QUAD_STORED is off).  The variants that differ from
    synth16x8's `-row` ones in the quad kernel alone run those paths alone: the others would run the `-row` variants' kernels a
    second time."""
    return v.problem == "synth16x8" and ("quad" in v.id or v.build == "lean")


def environment(monkeypatch, v):
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    for k, val in v.env.items():
        monkeypatch.setenv(k, val)


def solver(ilqg, v, entries, opts, groups=0, history=0):
    """a BatchSolver of variant v whose trajectory b starts from regtype2_cases.start(problem, fd, entries[b][0]); init() done"""
    st = [R.start(v.problem, v.fd, e[0]) for e in entries]
    B, params = len(st), st[0]["params"]
    s = ilqg.BatchSolver(v.problem, v.fd, batch=B, n_hor=st[0]["n_hor"], params=params, opts=dict(st[0]["opts"], **v.opts, **opts), strict=v.build, groups=groups)
    if v.rows == "car":  # a nominal table per trajectory: the rows twins, the same numbers
        s.set_params_batch({k: np.tile(np.asarray(params[k], dtype=np.float64), (B, 1)) for k in ("cu", "pf")})
    if v.rows == "almix":
        s.set_param_steps_batch("vref", np.tile(np.asarray(params["vref"], dtype=np.float64), (B, 1)))
    if history:
        s.set_history(history)
    restart(s, v, entries)
    return s


def restart(s, v, entries):
    st = [R.start(v.problem, v.fd, e[0]) for e in entries]
    s.init(np.array([t["x0"] for t in st]), np.array([t["u"] for t in st]))
    assert np.all(s.ints("status") == LC.ST_ACTIVE)


def enter(s, entries):
    s.set_scalar("lambda", np.array([e[1] for e in entries]))
    s.set_scalar("dlambda", np.array([e[2] for e in entries]))
    s.set_ints("need_derivs", 1)


def state(s, gains=True):
    out = {k: s.scalar(k).copy() for k in ("lambda", "dlambda", "g_norm", "dV0", "dV1", "cost")}
    out.update({k: s.ints(k).copy() for k in ("status", "iterations", "bp_calls", "bp_rc")})
    out["success"] = s.success()
    if gains:
        out["l"], out["L"] = s.gains()
    return out


def staged(s, entries, path, v=None):
    """one back_pass() from the entries: path "fused" (derivatives inside the sweep), "stored" (calc_derivs() first) or
    "records" (the CPU driver's derivative records put in place: the sweep's inputs are the reference's bit for bit)"""
    enter(s, entries)
    if path == "fused":
        s.back_pass(fused=True)
    elif path == "stored":
        s.calc_derivs()
        s.back_pass()
    else:
        st = [R.start(v.problem, v.fd, e[0]) for e in entries]
        s.set_derivs(np.array([t["rec"] for t in st]), np.array([t["fin"] for t in st]))
        s.back_pass()
    return state(s)


def own_records_are_the_references(s, v, entries):
    """whether calc_derivs() of this build leaves the CPU driver's records bit for bit (it does where the roll-out and the
    callbacks use no function the device evaluates in another form): then its sweeps have the reference's inputs too"""
    s.set_ints("need_derivs", 1)
    s.calc_derivs()
    rec, fin = s.derivs()
    st = [R.start(v.problem, v.fd, e[0]) for e in entries]
    return np.array_equal(rec, np.array([t["rec"] for t in st])) and np.array_equal(fin, np.array([t["fin"] for t in st]))


def held_back(got, b, e, sweep, exact, what, known=False):
    """slot b behind back_pass() against the expectation e (lambda_cases.expected) and the last sweep's gains"""
    ints = (int(got["status"][b]), int(got["bp_calls"][b]), int(got["bp_rc"][b]), int(got["iterations"][b]))
    assert ints == (e["status_back"], e["calls_back"], e["bp_rc_back"], 0), (what, ints, e["status_back"], e["calls_back"], e["bp_rc_back"])
    if not known:
        assert (got["lambda"][b], got["dlambda"][b]) == (e["lam_back"], e["dlam_back"]), (what, got["lambda"][b], got["dlambda"][b], e["lam_back"], e["dlam_back"])
    if e["bp_rc_back"] != 0:
        return 0.0
    pairs = [("g_norm", got["g_norm"][b], e["g_norm"]), ("dV0", got["dV0"][b], e["dV"][0]), ("dV1", got["dV1"][b], e["dV"][1]),
             ("l", got["l"][b], sweep["l"]), ("L", got["L"][b], sweep["L"])]
    dev = max(worst(a, r) for _, a, r in pairs)
    for k, a, r in pairs:
        assert (np.array_equal(a, r) if exact else worst(a, r) <= TOL), (what, k, worst(a, r))
    return dev


def held_end(got, b, e, what, known=False):
    """slot b behind iterate(1) under max_iter = 1: the whole of iLQG()"""
    ints = (int(got["status"][b]), int(got["success"][b]), int(got["iterations"][b]), int(got["bp_calls"][b]), int(got["bp_rc"][b]))
    assert ints == (e["status"], e["rc"], e["iterations"], e["calls_back"], e["bp_rc_back"]), (what, ints, e["status"], e["rc"], e["iterations"], e["calls_back"])
    if not known:
        assert (got["lambda"][b], got["dlambda"][b]) == (e["lam"], e["dlam"]), (what, got["lambda"][b], got["dlambda"][b], e["lam"], e["dlam"])


# every option a case may set, at the reference's defaults: one context serves all cases of a variant
BASE = dict(LC.DEFAULTS, lambdaInit=1.0, dlambdaInit=1.0, max_iter=1, fuse_derivs=1)
PATHS = ("records", "stored", "fused")


def configure(s, v, entry, opts):
    for k, val in dict(BASE, **opts).items():
        s.set_option(k, val)
    restart(s, v, [entry])


def device_g_norm(s, v, entry, opts, path):
    """g_norm of the sweep at the entry lambda in this build, on this path: a first device run that cannot exit"""
    configure(s, v, entry, dict(opts, tolGrad=NEVER))
    got = staged(s, [entry], path, v)
    assert got["bp_calls"][0] == 1 and got["bp_rc"][0] == 0 and got["status"][0] == LC.ST_ACTIVE
    return float(got["g_norm"][0])


# ---------------------------------------------------------------------------
# single cases
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("v", VARIANTS, ids=IDS)
def test_single_cases(ilqg, oracle_built, monkeypatch, v):
    """Bit for bit in the FMA-free builds wherever the sweep's inputs are the reference's: always on the path "records", and
    on the device's own derivatives where those leave the reference's records (own_records_are_the_references; not where the
    device evaluates a roll-out or a callback in another form than the host's libm: there the inputs differ in the last
    place and the doubles are held at the bar of the product builds)"""
    environment(monkeypatch, v)
    names = [n for n, c in LC.CASES.items() if (c["problem"], c["fd"]) == (v.problem, v.fd)]
    assert names
    top, same_inputs = 0.0, {}
    s = solver(ilqg, v, [(LC.CASES[names[0]]["first"], 1.0, 1.0)], BASE, history=2)
    for n in names:
        c = LC.CASES[n]
        entry = (c["first"], c["lam"], c["dlam"])
        known = n == LC.KNOWN_DIFFERENCE
        tie = c["opts"].get("tolGrad") in ("g", "g+")
        e = LC.expected(LC.case_run(n), c["lam"], c["dlam"])
        sweep = LC.sweep_of(c["problem"], c["fd"], c["first"], e["last_sweep_lambda"]) if e["bp_rc_back"] == 0 else None
        if c["first"] not in same_inputs:
            configure(s, v, entry, {})
            same_inputs[c["first"]] = own_records_are_the_references(s, v, [entry])
        for path in (("fused",) if transient_only(v) else PATHS):
            what = "%s %s %s" % (v.id, n, path)
            exact = v.build in EXACT and (path == "records" or same_inputs[c["first"]])
            o = dict(c["opts"], fuse_derivs=int(path == "fused"))
            if tie:
                o = LC.resolve(o, device_g_norm(s, v, entry, o, path))
            configure(s, v, entry, o)
            top = max(top, held_back(staged(s, [entry], path, v), 0, e, sweep, exact, what, known))
        # the whole loop, the entry through the options; fuse_derivs 1 (the default) and 0
        exact = v.build in EXACT and same_inputs[c["first"]]
        for fuse in ((1,) if transient_only(v) else (1, 0)):
            what = "%s %s iterate fuse_derivs %d" % (v.id, n, fuse)
            o = dict(c["opts"], fuse_derivs=fuse)
            if tie:
                o = LC.resolve(o, device_g_norm(s, v, entry, o, "fused" if fuse else "stored"))
            configure(s, v, entry, dict(o, lambdaInit=c["lam"], dlambdaInit=c["dlam"]))
            assert s.scalar("lambda")[0] == c["lam"] and s.scalar("dlambda")[0] == c["dlam"], what
            x, u, cost = s.x(), s.u(), s.scalar("cost").copy()
            s.iterate(1)
            got, n_hist = state(s, gains=False), s.history("n")["n"]
            held_end(got, 0, e, what, known)
            if e["status"] in (LC.ST_CONVERGED_GRAD, LC.ST_NO_DESCENT):  # no line search ran: nothing moved, nothing recorded
                assert np.array_equal(s.x(), x) and np.array_equal(s.u(), u) and np.array_equal(s.scalar("cost"), cost) and n_hist[0] == 0, what
            else:
                assert n_hist[0] == 1, what
            if e["bp_rc_back"] == 0:
                dev = max(worst(got["g_norm"][0], e["g_norm"]), worst(got["dV0"][0], e["dV"][0]), worst(got["dV1"][0], e["dV"][1]))
                assert dev == 0.0 if exact else dev <= TOL, (what, dev)
                top = max(top, dev)
    s.close()
    print("%s: %d cases, worst deviation of g_norm, dV and gains %.3g; own records are the reference's: %s" % (v.id, len(names), top, same_inputs))


# ---------------------------------------------------------------------------
# sequences: step 4 through the whole loop
# ---------------------------------------------------------------------------
SEQ_RUNS = [(n, v) for n, q in LC.SEQS.items() for v in VARIANTS if (v.problem, v.fd) == (q[0], q[1])]


@pytest.mark.parametrize("name,v", SEQ_RUNS, ids=["%s-%s" % (n, v.id) for n, v in SEQ_RUNS])
def test_sequences(ilqg, oracle_built, monkeypatch, name, v):
    """iterate(1) K times and solve(), fuse_derivs 1 and 0: behind iteration m what the reference's iLQG() returns with
    max_iter = m (a lane that goes on is ACTIVE where that run says MAX_ITER)"""
    environment(monkeypatch, v)
    problem, fd, first, opts, lam, dlam, K = LC.SEQS[name]
    runs = LC.seq_runs(name)
    es = [LC.expected(r, lam, dlam) for r in runs]
    top = 0.0
    for fuse in ((1,) if transient_only(v) else (1, 0)):
        what = "%s %s fuse_derivs %d" % (v.id, name, fuse)
        o = dict(opts, lambdaInit=lam, dlambdaInit=dlam, max_iter=K, fuse_derivs=fuse)
        s = solver(ilqg, v, [(first, lam, dlam)], o)
        for m in range(1, K + 1):
            live = s.ints("status")[0] == LC.ST_ACTIVE
            s.iterate(1)
            got, e = state(s, gains=False), es[m - 1]
            status = LC.ST_ACTIVE if (e["status"] == LC.ST_MAX_ITER and m < K) else e["status"]
            ints = (int(got["status"][0]), int(got["iterations"][0]))
            assert ints == (status, e["iterations"]) and (got["lambda"][0], got["dlambda"][0]) == (e["lam"], e["dlam"]), (what, m, ints, status, e["iterations"], got["lambda"][0], e["lam"], got["dlambda"][0], e["dlam"])
            if live:  # this iteration swept: as often as the reference's m-th
                calls = int(e["calls"][m - 1]) if len(e["calls"]) >= m else e["pending"]
                assert got["bp_calls"][0] == calls, (what, m, got["bp_calls"][0], calls)
                if e["bp_rc"] == 0:
                    dev = max(worst(got["g_norm"][0], e["g_norm"]), worst(got["dV0"][0], e["dV"][0]), worst(got["dV1"][0], e["dV"][1]), worst(got["cost"][0], e["cost"]))
                    assert dev <= TOL, (what, m, dev)  # (free-running from the device's own roll-outs: every build at the bar)
                    top = max(top, dev)
        s.close()
        s = solver(ilqg, v, [(first, lam, dlam)], o)
        s.solve()
        got, e = state(s, gains=False), es[-1]
        assert (int(got["status"][0]), int(got["success"][0]), int(got["iterations"][0]), got["lambda"][0], got["dlambda"][0]) == (e["status"], e["rc"], e["iterations"], e["lam"], e["dlam"]), (what, "solve")
        s.close()
    print("%s %s: worst deviation of g_norm, dV and cost %.3g" % (v.id, name, top))


# ---------------------------------------------------------------------------
# the drop-in host loop at B = 1
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("problem,fd", [("carparking", 0), ("carparking", 1), ("synth16x8", 1), ("synth10hx", 1)])
def test_drop_in_host_loop(ilqg, oracle_built, problem, fd):
    """the product's drop-in iLQG() (ilqg_host.c: retry loop, gradient exit, step 4) from every case's entry and through every
    sequence: return value, iterations and lambda exactly"""
    path = os.path.join(os.path.dirname(lib_path("oracle")), "libdrv_%s_fd%d_hip.so" % (problem, fd))

    def host(first, opts, lam, dlam, K):
        st = R.start(problem, fd, first)
        d = Driver(path, st["n_hor"], st["params"], dict(st["opts"], **opts, lambdaInit=lam, dlambdaInit=dlam, max_iter=K))
        assert d.init(st["x0"], st["u"]) == 1
        rc = d.solve()
        sc = d.scalars()
        d.close()
        return rc, int(sc["iterations"]), sc["lambda"], sc["g_norm"]

    n = 0
    for name, c in LC.CASES.items():
        if (c["problem"], c["fd"]) != (problem, fd):
            continue
        e = LC.case_run(name)
        opts = c["opts"]
        if opts.get("tolGrad") in ("g", "g+"):
            opts = LC.resolve(opts, host(c["first"], dict(opts, tolGrad=NEVER), c["lam"], c["dlam"], 1)[3])
        rc, its, lam, _ = host(c["first"], opts, c["lam"], c["dlam"], 1)
        assert (rc, its) == (e["rc"], e["iterations"]) and (lam == e["lam"] or name == LC.KNOWN_DIFFERENCE), (name, rc, its, lam, e["rc"], e["iterations"], e["lam"])
        n += 1
    for name, q in LC.SEQS.items():
        if (q[0], q[1]) != (problem, fd):
            continue
        for m, e in enumerate(LC.seq_runs(name), 1):
            rc, its, lam, _ = host(q[2], q[3], q[4], q[5], m)
            assert (rc, its, lam) == (e["rc"], e["iterations"], e["lam"]), (name, m, rc, its, lam, e["rc"], e["iterations"], e["lam"])
            n += 1
    assert n >= 8


# ---------------------------------------------------------------------------
# mixed batches
# ---------------------------------------------------------------------------
FIELDS = ("status", "iterations", "bp_calls", "bp_rc", "lambda", "dlambda")
SWEPT = ("g_norm", "dV0", "dV1", "l", "L")
BATCH_RUNS = [(n, v) for n, b in LC.BATCHES.items() for v in VARIANTS if (v.problem, v.fd) == (b[0], b[1])]


@pytest.mark.parametrize("name,v", BATCH_RUNS, ids=["%s-%s" % (n, v.id) for n, v in BATCH_RUNS])
def test_mixed_batches(ilqg, oracle_built, monkeypatch, name, v):
    """lanes of 1 to >= 5 sweeps, a no-descent lane and gradient-exit lanes side by side — the 64 lanes of a lane-mapped
    wavefront, the four rows of a quad wavefront — at B = 1, 5, 67 and 130, in order and reversed, over 1, 2 and 4 stream groups,
    and beside lanes that are already finished: every trajectory the reference's integers and lambdas, and bit for bit what
    it gives alone"""
    environment(monkeypatch, v)
    problem, fd, opts, lst = LC.BATCHES[name]
    runs = LC.batch_runs(name)
    es = [LC.expected(r, e[1], e[2]) for r, e in zip(runs, lst)]
    sweeps = [LC.sweep_of(problem, fd, e[0], x["last_sweep_lambda"]) if x["bp_rc_back"] == 0 else None for e, x in zip(lst, es)]
    n = len(lst)
    top = 0.0
    for path in (("fused",) if transient_only(v) else ("fused", "records")):
        fused = path == "fused"
        po = dict(opts, fuse_derivs=int(fused))
        alone = []
        s = solver(ilqg, v, lst[:1], po)
        for i, entry in enumerate(lst):  # (one context, started again for every entry)
            restart(s, v, [entry])
            same = v.build in EXACT and (not fused or own_records_are_the_references(s, v, [entry]))
            alone.append(staged(s, [entry], path, v))
            top = max(top, held_back(alone[i], 0, es[i], sweeps[i], same, "%s %s entry %d alone %s" % (v.id, name, i, path)))
        s.close()
        seen = set()
        for B in ((1, 5, 67, 130) if fused else (67,)):
            for reverse in (False, True):
                idx = [b % n for b in range(B)][::-1 if reverse else 1]
                for groups in ((1, 2, 4) if fused and B > 5 else (1,)):
                    what = "%s %s B %d %s groups %d %s" % (v.id, name, B, "reversed" if reverse else "in order", groups, path)
                    s = solver(ilqg, v, [lst[i] for i in idx], po, groups=groups)
                    seen.add(s.groups())
                    got = staged(s, [lst[i] for i in idx], path, v)
                    s.close()
                    for b, i in enumerate(idx):
                        for k in FIELDS + (SWEPT if es[i]["bp_rc_back"] == 0 else ()):
                            assert np.array_equal(got[k][b], alone[i][k][0]), (what, b, i, k, got[k][b], alone[i][k][0])
        assert len(seen) > 1 or not fused or problem != "carparking", seen
        # beside lanes that are already finished: those keep every field, the others are what they are alone
        B = 67
        idx = [b % n for b in range(B)]
        off = np.arange(B) % 3 == 1
        s = solver(ilqg, v, [lst[i] for i in idx], po)
        s.set_ints("status", np.where(off, LC.ST_MAX_ITER, LC.ST_ACTIVE).astype(np.int32))
        got = staged(s, [lst[i] for i in idx], path, v)
        s.close()
        for b, i in enumerate(idx):
            if off[b]:
                assert (got["status"][b], got["lambda"][b], got["dlambda"][b], got["iterations"][b]) == (LC.ST_MAX_ITER, lst[i][1], lst[i][2], 0), (v.id, name, b)
            else:
                for k in FIELDS + (SWEPT if es[i]["bp_rc_back"] == 0 else ()):
                    assert np.array_equal(got[k][b], alone[i][k][0]), (v.id, name, "beside finished lanes", b, i, k)
    # the whole loop on the widest batch: iterate(1) under max_iter = 1
    B = 130
    idx = [b % n for b in range(B)]
    s = solver(ilqg, v, [lst[i] for i in idx], dict(opts, max_iter=1), history=2)
    s.set_scalar("lambda", np.array([lst[i][1] for i in idx]))
    s.set_scalar("dlambda", np.array([lst[i][2] for i in idx]))
    x, u, cost = s.x(), s.u(), s.scalar("cost").copy()
    s.iterate(1)
    got, n_hist = state(s, gains=False), s.history("n")["n"]
    x1, u1 = s.x(), s.u()
    s.close()
    for b, i in enumerate(idx):
        held_end(got, b, es[i], "%s %s iterate slot %d entry %d" % (v.id, name, b, i))
        if es[i]["status"] in (LC.ST_CONVERGED_GRAD, LC.ST_NO_DESCENT):
            assert np.array_equal(x1[b], x[b]) and np.array_equal(u1[b], u[b]) and got["cost"][b] == cost[b] and n_hist[b] == 0, (v.id, name, b)
        else:
            assert n_hist[b] == 1, (v.id, name, b)
    print("%s %s: worst deviation of g_norm, dV and gains %.3g" % (v.id, name, top))
