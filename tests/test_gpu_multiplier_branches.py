"""The device's multiplier update and penalty schedule on each branch: the cases of tests/multiplier_cases.py (pinned to the
reference's own update_multipliers() and iLQG() by tests/test_multiplier_cases_recipe.py, no GPU) through the staged
update() — k_update, k_multipliers / k_multipliers_rows / the wave mapping's kernel, the cost-only roll-out — through init()
(the entry form), through iterate() (step 4 as sequences) and through the drop-in host loop.

A single update: init (the roll-out), set_multipliers, set_scalar of w_pen_l, w_pen_f, cost, new_cost, dcost, lambda, dlambda,
set_ints of accepted and status, update(), the reads.  set_scalar("w_pen_l") writes ILQG_F_WPEN_L alone, not
ILQG_F_WPEN_L_DER (ilqg_host.c scalar_names): nothing here reads the _DER fields before update() writes them itself
(k_multipliers' last two lines), and the sequences hold them through g_norm and dV of the sweeps behind a raise.

Compared per trajectory: both multiplier structs member by member, both weights, the re-swept cost, status, iterations and
lambda — bit for bit in the FMA-free libraries; in the product libraries weights and integers exactly and the doubles at the
suite's single-pass bar, 1e-10 relative to max(1, |ref|), the worst deviation printed.  ILQG_I_RESWEEP has no getter: that a
lane which is not active keeps RESWEEP = 0 shows in its cost, which the roll-out behind the update would otherwise replace."""
import os

import numpy as np
import pytest

import multiplier_cases as MC
from oracle.harness import Driver, lib_path

pytestmark = pytest.mark.gpu
TOL = 1e-10
N = MC.N
ACTIVE, CONVERGED_FUN, MAX_ITER = MC.ST_ACTIVE, MC.ST_CONVERGED_FUN, MC.ST_MAX_ITER
OUT = ("el", "fin", "wl", "wf", "cost", "new_cost", "lam", "status", "iterations")


@pytest.fixture(scope="module")
def ilqg():
    import __graft_entry__ as g
    g.build_for_tests()
    from ddp_generator_amd import ilqg as m
    if m.Problem("almix", 0).device_count() < 1:
        pytest.fail("no HIP device visible: the GPU tests must run on the MI355X box")
    return m


def worst(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.max(np.abs(a - b) / np.maximum(1.0, np.abs(b)))) if a.size else 0.0


def table(name):
    """(problem, params, options, reference) of a batch of single updates"""
    if name == "hli":
        return "brachi_hli", MC.brachi_hli_case(N)[0], MC.HLI_OPTS, MC.hli_reference()
    return "almix", MC.almix_params(N), MC.BATCHES[name][0], MC.reference(name)


def set_state(s, r, sel, role):
    """what the line search of an iteration would have left, per trajectory; role 0: accepted, 1: rejected, 2: accepted but
    finished (status MAX_ITER), 3: accepted with dcost below tolFun"""
    s.set_multipliers(r["el_in"][sel], r["fin_in"][sel])
    s.set_scalar("w_pen_l", r["w_in"][sel, 0])
    s.set_scalar("w_pen_f", r["w_in"][sel, 1])
    s.set_scalar("cost", r["cost_in"][sel])
    s.set_scalar("new_cost", r["new_cost"][sel])
    s.set_scalar("dcost", np.where(role == 3, 0.0, 1.0))
    s.set_scalar("lambda", 1.0)
    s.set_scalar("dlambda", 1.0)
    s.set_ints("iterations", 0)
    s.set_ints("accepted", (role != 1).astype(np.int32))
    s.set_ints("status", np.where(role == 2, MAX_ITER, ACTIVE).astype(np.int32))


def read(s):
    el, fin = s.multipliers()
    return dict(el=el, fin=fin, wl=s.scalar("w_pen_l"), wf=s.scalar("w_pen_f"), cost=s.scalar("cost"), new_cost=s.scalar("new_cost"), lam=s.scalar("lambda"),
                status=s.ints("status"), iterations=s.ints("iterations"), groups=s.groups())


def update(ilqg, name, build, fd=0, sel=None, role=None, groups=0, rows=None, twice=False):
    """one update() of the cases `sel` of batch `name` in library build `build` (False, True: FMA-free, "wave")"""
    problem, params, opts, r = table(name)
    sel = np.arange(len(r["cls"])) if sel is None else np.asarray(sel)
    role = np.zeros(len(sel), dtype=np.int32) if role is None else np.asarray(role)
    s = ilqg.BatchSolver(problem, fd, batch=len(sel), n_hor=N, params=params, opts=opts, strict=build, groups=groups)
    if rows is not None:
        s.set_params_batch({"tgt": rows["tgt"][sel]})
        s.set_param_steps_batch("vref", rows["vref"][sel])
    s.init(r["x0"][sel], r["u0"][sel])
    assert np.all(s.ints("status") == ACTIVE)
    set_state(s, r, sel, role)
    s.update()
    out = read(s)
    if twice:  # the same state set again in the used context
        set_state(s, r, sel, role)
        s.update()
        again = read(s)
        for k in OUT:
            assert np.array_equal(out[k], again[k]), ("second update in one context", k)
    s.close()
    return out


def held(r, out, sel, role, exact, what):
    """the comparison of the module docstring; returns the worst deviation of the compared doubles"""
    sel, role = np.asarray(sel), np.asarray(role)
    acc, rej, off, fun = role == 0, role == 1, role == 2, role == 3
    same = rej | off | fun  # no multiplier moves
    exp = dict(el=np.where(same[:, None, None], r["el_in"][sel], r["el"][sel]), fin=np.where(same[:, None], r["fin_in"][sel], r["fin"][sel]),
               wl=np.select([acc, rej], [r["w"][sel, 0], r["w_rej"][sel, 0]], r["w_in"][sel, 0]), wf=np.select([acc, rej], [r["w"][sel, 1], r["w_rej"][sel, 1]], r["w_in"][sel, 1]),
               cost=np.select([acc, rej, off], [r["cost"][sel], r["cost_rej"][sel], r["cost_in"][sel]], r["new_cost"][sel]), new_cost=r["new_cost"][sel],
               lam=np.select([rej, off], [1.6, 1.0], 1.0 / 1.6), status=np.select([off, fun], [MAX_ITER, CONVERGED_FUN], ACTIVE),
               iterations=np.where(off | fun, 0, 1))
    for k in ("wl", "wf", "status", "iterations", "new_cost", "lam"):
        assert np.array_equal(out[k], exp[k]), (what, k, out[k], exp[k])
    # what does not take the update or the re-sweep comes back untouched, in every build
    assert np.array_equal(out["el"][same], exp["el"][same]) and np.array_equal(out["fin"][same], exp["fin"][same]), what
    assert np.array_equal(out["cost"][off | fun], exp["cost"][off | fun]), what
    dev = {k: worst(out[k], exp[k]) for k in ("el", "fin", "cost")}
    print("%s: worst deviation " % what + ", ".join("%s %.3g" % kv for kv in dev.items()))
    if exact:
        bad = [(int(sel[b]), r["cls"][sel[b]]) for b in range(len(sel)) if not (np.array_equal(out["el"][b], exp["el"][b]) and np.array_equal(out["fin"][b], exp["fin"][b]) and out["cost"][b] == exp["cost"][b])]
        assert not bad, (what, bad)
    else:
        assert max(dev.values()) <= TOL, (what, dev)
    return max(dev.values())


@pytest.mark.parametrize("strict", [True, False])
@pytest.mark.parametrize("fd", [0, 1])
@pytest.mark.parametrize("name", list(MC.BATCHES))
def test_single_updates(ilqg, name, fd, strict):
    """every case accepted: update_multipliers(o, 0) and the re-sweep (iLQG.c:337-338), the whole table one batch"""
    r = MC.reference(name)
    B = len(r["cls"])
    assert B % 64 != 0
    out = update(ilqg, name, strict, fd)
    held(r, out, np.arange(B), np.zeros(B, dtype=np.int32), strict, "%s fd%d %s" % (name, fd, "FMA-free" if strict else "product"))


@pytest.mark.parametrize("strict", [True, False])
@pytest.mark.parametrize("name", ["free", "caps"])
def test_lane_patterns_of_accepted_and_status(ilqg, name, strict):
    """neighbouring lanes accepted / rejected / finished / leaving on tolFun, every case in every role in turn: accepted lanes
    take the update, rejected ones w fact2 clamped and the re-sweep (the reference side: set_state with the raised weights,
    cost_resweep()), lanes that are not active come back untouched in every field"""
    r = MC.reference(name)
    B = len(r["cls"])
    for shift in range(4):
        role = (np.arange(B) + shift) % 4
        out = update(ilqg, name, strict, 0, role=role)
        held(r, out, np.arange(B), role, strict, "%s roles + %d %s" % (name, shift, "FMA-free" if strict else "product"))


@pytest.mark.parametrize("strict", [True, False])
def test_identities(ilqg, strict):
    """bit for bit in every build: the batch reversed, one trajectory alone, 1, 2 and 4 stream groups, a second update() in a
    used context against a fresh one"""
    r = MC.reference("free")
    B = len(r["cls"])
    role = (np.arange(B) % 4 == 1).astype(np.int32)  # (every fourth lane rejected)
    base = update(ilqg, "free", strict, role=role, groups=1, twice=True)
    rev = update(ilqg, "free", strict, sel=np.arange(B)[::-1], role=role[::-1], groups=1)
    for k in OUT:
        assert np.array_equal(base[k], rev[k][::-1]), ("reversed", k)
    seen = {base["groups"]}
    for groups in (2, 4):
        out = update(ilqg, "free", strict, role=role, groups=groups)
        seen.add(out["groups"])
        for k in OUT:
            assert np.array_equal(base[k], out[k]), ("groups", groups, k)
    assert len(seen) > 1, seen
    for b in (1, 6, B - 1):
        one = update(ilqg, "free", strict, sel=[b], role=role[b:b + 1])
        for k in OUT:
            assert np.array_equal(base[k][b], one[k][0]), ("B = 1", b, k)


@pytest.mark.parametrize("strict", [True, False])
def test_rows_twin(ilqg, strict):
    """k_multipliers_rows: one trajectory in every slot, a tgt row and a vref window per slot (hfi and hli_1 exactly zero, either
    side of the tolerance and of the stall test), every slot against a Driver under that slot's own parameters; and nominal
    rows equal to the shared batch bit for bit"""
    r = MC.rows_reference()
    B = MC.ROWS_B
    problem, params, opts = "almix", MC.almix_params(N), MC.ROWS_OPTS
    s = ilqg.BatchSolver(problem, 0, batch=B, n_hor=N, params=params, opts=opts, strict=strict)
    s.set_params_batch({"tgt": r["tgt"]})
    s.set_param_steps_batch("vref", r["vref"])
    s.init(r["x0"], r["u0"])
    assert np.all(s.ints("status") == ACTIVE)
    role = np.zeros(B, dtype=np.int32)
    set_state(s, r, np.arange(B), role)
    s.update()
    out = read(s)
    s.close()
    held(r, out, np.arange(B), role, strict, "rows %s" % ("FMA-free" if strict else "product"))
    if strict:  # the exact zeros are zeros on the device
        z = [b for b, c in enumerate(r["cls"]) if c == "hfi_zero"]
        assert len(z) >= 2 and np.all(out["fin"][z, 5] == 0.0) and np.all(out["fin"][z, 4] == r["fin_in"][z, 4])
    f = MC.reference("free")
    Bf = len(f["cls"])
    shared = update(ilqg, "free", strict)
    nominal = update(ilqg, "free", strict, rows=dict(tgt=np.tile(np.array(MC.TGT), (Bf, 1)), vref=np.tile(params["vref"], (Bf, 1))))
    for k in OUT:
        assert np.array_equal(shared[k], nominal[k]), ("nominal rows", k)


@pytest.mark.parametrize("build", [True, False, "wave"])
def test_brachi_hli_updates(ilqg, build):
    """the problem of the wave mapping (one running inequality, one final equality) through the lane-mapped libraries and
    through the wave build, which exists as a product build only"""
    r = MC.hli_reference()
    B = MC.HLI_B
    for shift in (0, 1):
        role = ((np.arange(B) + shift) % 2) * np.int32(shift > 0)  # all accepted, then every other lane rejected
        out = update(ilqg, "hli", build, role=role)
        held(r, out, np.arange(B), role, build is True, "brachi_hli %s roles %d" % (build, shift))


@pytest.mark.parametrize("build", [True, False, "wave"])
def test_entry_form(ilqg, build):
    """after init(): last_h* of step 0 only, steps 1.. as init_multipliers() left them, last_hf*, no mu and no weight moved"""
    top = 0.0
    for (tag, problem, params, opts, x0, u0), e in zip(MC.entry_cases(), MC.entry_reference().values()):
        if build == "wave" and problem != "brachi_hli":
            continue
        s = ilqg.BatchSolver(problem, 0, batch=len(x0), n_hor=N, params=params, opts=opts, strict=build)
        s.init(x0, u0)
        el, fin = s.multipliers()
        w = np.stack([s.scalar("w_pen_l"), s.scalar("w_pen_f")], axis=1)
        cost = s.scalar("cost")
        s.close()
        assert np.array_equal(w, e["w"]) and el.shape == e["el"].shape, tag
        dev = max(worst(el, e["el"]), worst(fin, e["fin"]), worst(cost, e["cost"]))
        top = max(top, dev)
        if build is True:
            assert np.array_equal(el, e["el"]) and np.array_equal(fin, e["fin"]) and np.array_equal(cost, e["cost"]), tag
        else:
            assert dev <= TOL, (tag, dev)
            # what the entry form must not touch is exact in every build
            assert np.array_equal(el[:, 1:], e["el"][:, 1:]) and np.array_equal(el == 0.0, e["el"] == 0.0) and np.array_equal(fin == 0.0, e["fin"] == 0.0), tag
    print("entry form %s: worst deviation %.3g" % (build, top))


def run_sequence(ilqg, name, fd, strict, fuse):
    opts, K = MC.SEQ[name]
    x0, u0 = MC.seq_start()
    B = 2
    s = ilqg.BatchSolver("almix", fd, batch=B, n_hor=MC.SEQ_N, params=MC.almix_params(MC.SEQ_N), opts=dict(opts, max_iter=K, fuse_derivs=fuse), strict=strict)
    s.init(np.tile(x0, (B, 1)), np.tile(u0, (B, 1, 1)))
    hist = [dict(cost=s.scalar("cost"))]
    for _ in range(K):
        s.iterate(1)
        hist.append({k: s.scalar(k) for k in ("cost", "w_pen_l", "w_pen_f", "lambda", "g_norm", "dV0", "dV1")} | {k: s.ints(k) for k in ("status", "iterations")})
    el, fin = s.multipliers()
    hist.append(dict(el=el, fin=fin, success=s.success()))
    s.close()
    return hist


@pytest.mark.parametrize("strict", [True, False])
@pytest.mark.parametrize("fd", [0, 1])
@pytest.mark.parametrize("name", list(MC.SEQ))
def test_step_4_sequences(ilqg, name, fd, strict):
    """iterate(1) K times under options that force the branch (every search rejected by alpha = [0.0]; caps; the lambdaMax
    exit behind a raise; w_pen_fact2 = 1; the tolFun exit; max_iter on an accepted iteration): every iteration's cost,
    weights, lambda, g_norm, dV, iterations and status (ACTIVE, then MAX_ITER, LAMBDA_MAX or CONVERGED_FUN by value, as the
    reference's runs imply them: MC.sequence_reference) against the reference's solve with that max_iter and its trace, the
    last state against the longest solve; fuse_derivs 1 and 0 the same bits"""
    ref = MC.sequence_reference(name, fd)
    K = MC.SEQ[name][1]
    runs = [run_sequence(ilqg, name, fd, strict, fuse) for fuse in (1, 0)]
    T = len(ref["trace_g_norm"])
    top = 0.0
    for fuse, hist in zip((1, 0), runs):
        what = "%s fd%d %s fuse_derivs %d" % (name, fd, "FMA-free" if strict else "product", fuse)
        pairs = [("init_cost", hist[0]["cost"], ref["init_cost"])]
        for j in range(K):
            h, t = hist[j + 1], min(j, T - 1)
            assert np.all(h["w_pen_l"] == ref["w"][j, 0]) and np.all(h["w_pen_f"] == ref["w"][j, 1]) and np.all(h["iterations"] == ref["iterations"][j]), (what, j, h)
            assert np.all(h["status"] == ref["status"][j]), (what, j, h["status"], ref["status"][j])
            pairs += [("cost", h["cost"], ref["cost"][j]), ("lambda", h["lambda"], ref["lambda"][j]), ("g_norm", h["g_norm"], ref["trace_g_norm"][t]),
                      ("dV0", h["dV0"], ref["trace_dV0"][t]), ("dV1", h["dV1"], ref["trace_dV1"][t])]
        last = hist[-1]
        assert np.all(last["success"] == ref["rc"][K - 1]), (what, last["success"])
        pairs += [("el", last["el"], ref["el"][K - 1][None]), ("fin", last["fin"], ref["fin"][K - 1][None])]
        dev = {}
        for k, a, b in pairs:
            dev[k] = max(dev.get(k, 0.0), worst(a, np.broadcast_to(b, np.shape(a))))
            assert (np.all(np.asarray(a) == b) if strict else dev[k] <= TOL), (what, k, a, b)
        print("%s: worst deviation " % what + ", ".join("%s %.3g" % kv for kv in dev.items()))
        top = max(top, max(dev.values()))
    if name == "rej_fact2_1":  # no weight moves: the cost is the initial cost's bits in every build
        assert all(np.all(h["cost"] == runs[0][0]["cost"]) for h in runs[0][1:-1])
    for a, b in zip(*runs):
        for k in a:
            assert np.array_equal(a[k], b[k]), (name, fd, strict, "fuse_derivs 1 against 0", k)


def test_drop_in_host_loop(ilqg, oracle_built):
    """the host loop of the product's drop-in iLQG() (accept / update / re-sweep, reject / raise / re-sweep / lambdaMax exit) on
    the rejection sequences: the reference's iterations, return code and weights exactly, its cost at the bar"""
    path = os.path.join(os.path.dirname(lib_path("oracle")), "libdrv_almix_fd0_hip.so")
    top = 0.0
    for name in ("rej3", "rej3_caps", "rej_lambda_max", "rej_fact2_1", "rej_above_cap"):
        opts, K = MC.SEQ[name]
        ref = MC.sequence_reference(name, 0)
        for m in range(1, K + 1):
            d = Driver(path, MC.SEQ_N, MC.almix_params(MC.SEQ_N), dict(opts, max_iter=m))
            assert d.init(*MC.seq_start()) == 1
            rc = d.solve()
            sc, w = d.scalars(), d.multipliers()[2]
            d.close()
            assert (rc, sc["iterations"], w) == (ref["rc"][m - 1], ref["iterations"][m - 1], tuple(ref["w"][m - 1])), (name, m, rc, sc, w)
            dev = worst(sc["cost"], ref["cost"][m - 1])
            top = max(top, dev)
            assert dev <= TOL, (name, m, dev)
    print("drop-in host loop: worst deviation of the cost %.3g" % top)
