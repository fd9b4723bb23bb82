"""What tests/test_gpu_multiplier_branches.py compares the device's multiplier update and penalty schedule against, pinned to
the reference's own update_multipliers() and iLQG() (no GPU): on every case of tests/multiplier_cases.py the CPU restatement
gives what tests/golden/multipliers.npz records of the reference build, bit for bit — and, where the reference build
oracle/_ref exists, what that build gives live.  The table's own conditions (the stalls that happen are the ones each case
names, margins of the tolerance and of the stall test, every class populated as labelled) are asserted on the same numbers,
and restatements of the update (numpy) and of step 4 (the driver's single stages) with switchable mistakes show that each
mistake is caught by at least one case."""
import os

import numpy as np
import pytest

import multiplier_cases as MC
from conftest import golden
from oracle.harness import Driver, lib_path

NAMES = list(MC.BATCHES)
N = MC.N
HAVE_REF = os.path.exists(lib_path("ref", "almix", 0))


def flat_golden(prefix):
    g = golden("multipliers.npz")
    return {k[len(prefix):]: g[k] for k in g.files if k.startswith(prefix)}


def test_the_golden_holds_nothing_else(oracle_built):
    assert set(golden("multipliers.npz").files) == set(MC.golden_of("oracle"))
    assert os.path.getsize(MC.GOLDEN) < 256 * 1024


@pytest.mark.parametrize("name", NAMES)
def test_oracle_gives_the_reference_builds_bits(oracle_built, name):
    g, r = flat_golden(name + "/"), MC.reference(name)
    assert len(g) == 8
    for k, v in g.items():
        assert np.array_equal(r[k], v), (name, k)
    r1 = MC.reference(name, "oracle", 1)  # (the update does not depend on FULL_DDP: the fd1 libraries are held to the same table)
    for k in MC.FIELDS:
        assert np.array_equal(r[k], r1[k]), (name, k)
    if HAVE_REF:
        live = MC.reference(name, "ref")
        for k in MC.FIELDS:
            assert np.array_equal(r[k], live[k]), (name, k)


def test_rows_entry_and_sequences_give_the_reference_builds_bits(oracle_built):
    kinds = ("oracle", "ref") if HAVE_REF else ("oracle",)
    for kind in kinds:
        g, r = flat_golden("rows/"), MC.rows_reference(kind)
        assert len(g) == 6 and all(np.array_equal(r[k], v) for k, v in g.items()), kind
        for tag, e in MC.entry_reference(kind).items():
            g = flat_golden("entry_%s/" % tag)
            assert set(g) == set(e) and all(np.array_equal(e[k], v) for k, v in g.items()), (kind, tag)
        for name in MC.SEQ:
            for fd in (0, 1):
                g, s = flat_golden("seq_%s_fd%d/" % (name, fd)), MC.sequence_reference(name, fd, kind)
                assert set(g) == set(s) and all(np.array_equal(np.asarray(s[k]), v) for k, v in g.items()), (kind, name, fd)


# ---------------------------------------------------------------------------
# update_multipliers() restated (problems/almix/iLQG_func.c:584-660), with the mistakes a device form could make
# ---------------------------------------------------------------------------
UPDATE_MUTATIONS = ("raise_per_step", "last_step_forgotten", "fabs_on_inequality", "no_fabs_on_equality", "no_tolerance", "stored_before_compared",
                    "not_stored", "caps_swapped", "no_cap_l", "no_cap_f", "above_cap_left_alone", "mu_fe_with_raised_weight", "either_raises_both")
INIT_MUTATIONS = ("init_walks_every_step", "init_raises_a_weight")


def update_np(h_run, h_fin, el, fin, w, o, init=0, mut=None):
    """(el, fin, (w_pen_l, w_pen_f), stalled) — stalled: the set of triggers ("hle", 0, k) ... ("hfi", 0) whose test came out
    true.  The arithmetic in the generated file's order (no contraction: the CPU builds are FMA-free)"""
    el, fin = np.array(el, dtype=np.float64), np.array(fin, dtype=np.float64)
    wl, wf = float(w[0]), float(w[1])
    stalled = set()

    def stalls(kind, v, last):
        if (kind == "e" and mut != "no_fabs_on_equality") or (kind == "i" and mut == "fabs_on_inequality"):
            v, last = abs(v), abs(last)
        return (mut == "no_tolerance" or v > o["tol"]) and o["fact1"] * v > last

    def active(mu, h, wp):
        return mu * (2.0 * h * wp + 1.0) if (h > 0 if mut == "gt_for_ge" else h >= 0) else mu / ((-h * wp + 1.0) * (-h * wp + 1.0))
    for k in range(len(h_run)):
        for j, (name, i, kind, cmu, clast) in enumerate(MC.RUNNING):
            h = h_run[k, j]
            if stalls(kind, h, h if mut == "stored_before_compared" else el[k, clast]):
                stalled.add((name, i, k))
            if mut != "not_stored":
                el[k, clast] = h
        if init:
            if mut == "init_walks_every_step":
                continue
            break
        el[k, 0] = h_run[k, 0] * wl + el[k, 0]
        el[k, 2] = active(el[k, 2], h_run[k, 1], wl)
        el[k, 3] = active(el[k, 3], h_run[k, 2], wl)
    for j, (name, i, kind, cmu, clast) in enumerate(MC.FINAL):
        if stalls(kind, h_fin[j], h_fin[j] if mut == "stored_before_compared" else fin[clast]):
            stalled.add((name, i))
        if mut != "not_stored":
            fin[clast] = h_fin[j]
    steps = sorted({t[2] for t in stalled if len(t) == 3})
    if mut == "last_step_forgotten":
        steps = [k for k in steps if k != len(h_run) - 1]
    run_st, fin_st = len(steps) > 0, any(len(t) == 2 for t in stalled)
    if mut == "either_raises_both":
        run_st = fin_st = run_st or fin_st
    max_l, max_f = (o["max_f"], o["max_l"]) if mut == "caps_swapped" else (o["max_l"], o["max_f"])

    def raised(wp, cap, no_cap):
        if mut == "above_cap_left_alone" and wp > cap:
            return wp
        return wp * o["fact1"] if no_cap else min(cap, wp * o["fact1"])
    wl_new, wf_new = wl, wf
    if (not init or mut == "init_raises_a_weight") and run_st:
        for _ in range(len(steps) if mut == "raise_per_step" else 1):
            wl_new = raised(wl_new, max_l, mut == "no_cap_l")
    if (not init or mut == "init_raises_a_weight") and fin_st:
        wf_new = raised(wf, max_f, mut == "no_cap_f")
    if not init:
        wp = wf_new if mut == "mu_fe_with_raised_weight" else wf
        fin[0] = h_fin[0] * wp + fin[0]
        fin[1] = h_fin[1] * wp + fin[1]
        fin[4] = active(fin[4], h_fin[2], wf)
    return el, fin, (wl_new, wf_new), stalled


def margins_hold(h_run, h_fin, el_in, fin_in, o, what):
    """no violation within 1e-6 relative of the tolerance, no fact1 v within 1e-6 relative of the remembered value — every
    constraint of every step and of the final part; returns the number of exact zeros, which are left out"""
    pairs = [(kind, h_run[k, j], el_in[k, clast]) for k in range(len(h_run)) for j, (_, _, kind, _, clast) in enumerate(MC.RUNNING)]
    pairs += [(kind, h_fin[j], fin_in[clast]) for j, (_, _, kind, _, clast) in enumerate(MC.FINAL)]
    zeros = 0
    for kind, v, last in pairs:
        if kind == "e":
            v, last = abs(v), abs(last)
        if v == 0.0:
            zeros += 1
            continue
        assert abs(v - o["tol"]) > MC.MARGIN * o["tol"] and abs(o["fact1"] * v - last) > MC.MARGIN * abs(last), (what, v, last)
    return zeros


def restated(name, mut=None):
    r, o = MC.reference(name), MC.options(name)
    return [update_np(r["h_run"][b], r["h_fin"][b], r["el_in"][b], r["fin_in"][b], r["w_in"][b], o, 0, mut) for b in range(len(r["cls"]))]


def differs(a, b):
    return not (np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and tuple(a[2]) == tuple(b[2]))


@pytest.mark.parametrize("name", NAMES)
def test_restated_update_equals_the_reference(oracle_built, name):
    r = MC.reference(name)
    for b, out in enumerate(restated(name)):
        assert not differs(out, (r["el"][b], r["fin"][b], r["w"][b])), (name, b, r["cls"][b])


@pytest.mark.parametrize("name", NAMES)
def test_table_meets_its_conditions(oracle_built, name):
    r, o = MC.reference(name), MC.options(name)
    B = len(r["cls"])
    assert B == MC.BATCHES[name][2] and B % 64 != 0 and B <= 130
    assert np.all(r["el_in"][:, :, [0, 2, 3]] != 0.0) and np.all(r["fin_in"][:, [0, 1, 4]] != 0.0)  # non-zero mu throughout
    outs = restated(name)
    by = {}
    for b, c_name in enumerate(r["cls"]):
        by.setdefault(c_name, []).append(b)
        c, st = r["case"][b], outs[b][3]
        # the stalls that happen are exactly the ones the case names
        assert st == set(c["stall"]), (name, b, c_name, st)
        # margins: every compared quantity 1e-6 relative away from the tolerance and from the remembered value
        zeros = margins_hold(r["h_run"][b], r["h_fin"][b], r["el_in"][b], r["fin_in"][b], o, (name, b))
        assert zeros == (1 if c_name == "zero_hli" else 0)
    assert set(by) == set(MC.BATCHES[name][1])
    f1 = o["fact1"]
    for c_name, bs in by.items():
        assert len(bs) >= 2, c_name
        assert len({id(r["case"][b]) for b in bs}) == len(MC.BATCHES[name][1][c_name])  # every case of the class is in the batch
        for b in bs:
            c, st = r["case"][b], outs[b][3]
            w_in, w = tuple(r["w_in"][b]), tuple(r["w"][b])
            steps, fin = {t[2] for t in st if len(t) == 3}, {t for t in st if len(t) == 2}
            what = (name, b, c_name)
            if c_name in ("none", "tol_inside", "ineq_negative", "zero_hli", "above_cap_quiet", "f1_none"):
                assert not st and w == w_in, what
            if c_name == "step_first":
                assert steps == {0} and not fin and w == (w_in[0] * f1, w_in[1]), what
            elif c_name == "step_middle":
                assert len(steps) == 1 and 0 < min(steps) < N - 1 and not fin and w == (w_in[0] * f1, w_in[1]), what
            elif c_name == "step_last":
                assert steps == {N - 1} and not fin and w == (w_in[0] * f1, w_in[1]), what
            elif c_name == "steps_several":
                assert len(steps) >= 2 and not fin and w == (w_in[0] * f1, w_in[1]), what
            elif c_name == "final_only":
                assert not steps and fin and w == (w_in[0], w_in[1] * f1), what
            elif c_name in ("both_parts", "f1_stall"):
                assert steps and fin and w == (w_in[0] * f1, w_in[1] * f1), what
            elif c_name.startswith("only_"):
                kind, i = c_name[5:8], int(c_name[8])
                assert len(st) == 1 and next(iter(st))[:2] == (kind, i), what
            elif c_name in ("tol_inside", "tol_outside"):
                h, lo, hi = r["h_run"][b, 0, 1], o["tol"] * (1 - 8 * MC.NEAR), o["tol"] * (1 + 8 * MC.NEAR)
                assert 0 < r["el_in"][b, 0, 4] < h and ((lo < h < o["tol"]) if c_name == "tol_inside" else (o["tol"] < h < hi and st == {("hli", 0, 0)})), what
            elif c_name == "eq_negative":
                (t,) = st
                assert t[0] in ("hle", "hfe") and (r["h_run"][b, t[2], 0] if len(t) == 3 else r["h_fin"][b, t[1]]) < 0, what
            elif c_name == "ineq_negative":
                for t in c["last"]:
                    h, last = (r["h_run"][b, t[2], 1 + t[1]], r["el_in"][b, t[2], 4 + t[1]]) if len(t) == 3 else (r["h_fin"][b, 2], r["fin_in"][b, 5])
                    assert h < last < 0, what  # negative, and larger in magnitude than the one remembered
            elif c_name == "zero_hli":
                assert r["h_run"][b, 0, 1] == 0.0 and r["el"][b, 0, 2] == r["el_in"][b, 0, 2], what
            elif c_name == "uncapped":
                assert w == (w_in[0] * f1, w_in[1] * f1) and w[0] < o["max_l"] and w[1] < o["max_f"], what
            elif c_name == "l_capped_only":
                assert w == (o["max_l"], w_in[1] * f1) and w_in[0] * f1 > o["max_l"] and w[1] < o["max_f"], what
            elif c_name == "f_capped_only":
                assert w == (w_in[0] * f1, o["max_f"]) and w_in[1] * f1 > o["max_f"] and w[0] < o["max_l"], what
            elif c_name == "both_capped":
                assert w == (o["max_l"], o["max_f"]) and w_in[0] < o["max_l"] and w_in[1] < o["max_f"], what
            elif c_name == "at_cap":
                assert st and w == w_in and (w_in[0] == o["max_l"] or w_in[1] == o["max_f"]), what
            elif c_name in ("above_cap_stall", "f1_above_cap"):
                assert st and w == (o["max_l"] if steps else w_in[0], o["max_f"] if fin else w_in[1]) and w != w_in, what
                assert (w_in[0] > o["max_l"] if steps else True) and (w_in[1] > o["max_f"] if fin else True), what
    if name == "free":  # one running step alone: the first, a middle one and the last, each by itself; each constraint the only trigger
        assert {c for c in by} >= {"step_first", "step_middle", "step_last", "only_hle0", "only_hli0", "only_hli1", "only_hfe0", "only_hfe1", "only_hfi0"}
    # a rejected step's raise, as the reference's two lines state it
    assert np.array_equal(r["w_rej"][:, 0], np.minimum(o["max_l"], r["w_in"][:, 0] * o["fact2"])) and np.array_equal(r["w_rej"][:, 1], np.minimum(o["max_f"], r["w_in"][:, 1] * o["fact2"]))
    # the re-swept costs tell the cases apart (a lane reading its neighbour's state would show)
    assert len(set(r["cost"])) == B and len(set(r["cost_rej"])) == B and np.all(r["cost"] != r["new_cost"])


ROWS_EXPECT = dict(nominal="", hfi_zero="", hfi_inside="", hfi_outside="f", hfi_beyond="f", hfi_negative="", hli_zero="", hli_inside="", hli_outside="l",
                   hli_negative="", vref_high="l", vref_low="l", cost_only="")


def test_rows_table_meets_its_conditions(oracle_built):
    r = MC.rows_reference()
    o = dict(tol=MC.TOL_DEFAULT, fact1=MC.FACT1_DEFAULT, max_l=np.inf, max_f=np.inf)
    assert len(r["cls"]) == MC.ROWS_B and MC.ROWS_B % 64 != 0 and set(r["cls"]) == set(ROWS_EXPECT)
    for b, c_name in enumerate(r["cls"]):
        out = update_np(r["h_run"][b], r["h_fin"][b], r["el_in"][b], r["fin_in"][b], r["w_in"][b], o)
        assert not differs(out, (r["el"][b], r["fin"][b], r["w"][b])), (b, c_name)
        # the margins of EVERY constraint under the slot's own row, against the tolerance and against the remembered value
        assert margins_hold(r["h_run"][b], r["h_fin"][b], r["el_in"][b], r["fin_in"][b], o, ("rows", b)) == (1 if c_name in ("hfi_zero", "hli_zero") else 0)
        w_in, w = r["w_in"][b], r["w"][b]
        assert (w[0] != w_in[0], w[1] != w_in[1]) == ("l" in ROWS_EXPECT[c_name], "f" in ROWS_EXPECT[c_name]), (b, c_name)
        tol = o["tol"]
        if c_name == "hfi_zero":
            assert r["h_fin"][b, 2] == 0.0
        elif c_name in ("hfi_inside", "hfi_outside"):
            assert abs(r["h_fin"][b, 2] - tol) > MC.MARGIN * tol and abs(r["h_fin"][b, 2] - tol) < 8 * MC.NEAR * tol
        elif c_name == "hli_zero":
            assert r["h_run"][b, 0, 1] == 0.0
        elif c_name in ("hli_inside", "hli_outside"):
            assert abs(r["h_run"][b, 0, 1] - tol) > MC.MARGIN * tol and abs(r["h_run"][b, 0, 1] - tol) < 8 * MC.NEAR * tol
        elif c_name == "vref_high":
            assert np.all(r["h_run"][b, :, 0] < 0)
        elif c_name == "vref_low":
            assert np.all(r["h_run"][b, :, 0] > 0)
    nominal = [b for b, c in enumerate(r["cls"]) if c == "nominal"]
    assert nominal[0] == 0 and np.array_equal(r["tgt"][0], MC.TGT) and np.array_equal(r["vref"][0], MC.almix_params(N)["vref"])
    assert np.all(r["x"] == r["x"][0]) and np.all(r["u"] == r["u"][0])  # one trajectory in every slot
    assert len(set(r["cost"])) == MC.ROWS_B


def test_brachi_hli_table(oracle_built):
    """the wave mapping's problem: the oracle's bits are the golden's (and the live reference build's), and every class does
    what its label says"""
    g, r = flat_golden("hli/"), MC.hli_reference()
    assert len(g) == 8 and all(np.array_equal(r[k], v) for k, v in g.items())
    if HAVE_REF:
        live = MC.hli_reference("ref")
        assert all(np.array_equal(r[k], live[k]) for k in MC.FIELDS)
    assert set(r["cls"]) == set(MC.HLI_CLASSES) and MC.HLI_B % 64 != 0
    f1 = MC.FACT1_DEFAULT
    for b, c_name in enumerate(r["cls"]):
        run, fin = r["stalls"][b]
        w_in, w = r["w_in"][b], r["w"][b]
        assert w[0] == (min(MC.HLI_OPTS["w_pen_max_l"], w_in[0] * f1) if run else w_in[0]) and w[1] == (w_in[1] * f1 if fin else w_in[1]), (b, c_name)
        assert np.all(r["el_in"][b, :, 0] != 0.0) and np.array_equal(r["el"][b, :, 1], r["h_run"][b, :, 0]) and r["fin"][b, 1] == r["h_fin"][b, 0]
        # margins of the stall test (every |h| is far above the tolerance)
        v, last = r["h_run"][b, :, 0], r["el_in"][b, :, 1]
        assert np.all(np.abs(v) > 1e-3) and np.all(np.abs(f1 * v - last) > MC.MARGIN * np.abs(last)) and abs(f1 * abs(r["h_fin"][b, 0]) - abs(r["fin_in"][b, 1])) > MC.MARGIN
        if c_name == "neg_growing":
            neg = v < 0
            assert neg.sum() >= 4 and np.all(v[neg] < last[neg]) and np.all(last[neg] < 0) and not run
        if c_name in ("run_first", "run_last", "both"):
            assert run and np.sum(0.5 * v == last) == (2 if c_name == "both" else 1)
    assert len(set(r["cost"])) == MC.HLI_B


def entry_inputs():
    """per almix entry start: (h_run, h_fin) and the structs init_multipliers() leaves (iLQG_func.c:546-565)"""
    tag, problem, params, opts, x0, u0 = MC.entry_cases()[0]
    el0, fin0 = np.zeros((N, 6)), np.zeros(6)
    el0[:, 2:4], fin0[4] = 1.0, 1.0
    return [(MC.values("oracle", 0, params, opts, x0[b], u0[b])[:2], el0, fin0) for b in range(len(x0))]


def test_entry_form(oracle_built):
    """last_h* of step 0 only, steps 1.. as init_multipliers() left them, last_hf* of the final part, no mu and no weight moved
    although step 0 stalls"""
    e = MC.entry_reference()
    o = dict(tol=MC.TOL_DEFAULT, fact1=MC.FACT1_DEFAULT, max_l=np.inf, max_f=np.inf)
    a = e["almix"]
    for b, ((h_run, h_fin), el0, fin0) in enumerate(entry_inputs()):
        el, fin, w, st = update_np(h_run, h_fin, el0, fin0, MC.ENTRY_W, o, init=1)
        assert np.array_equal(el, a["el"][b]) and np.array_equal(fin, a["fin"][b]) and w == tuple(a["w"][b]) == MC.ENTRY_W, b
        assert any(len(t) == 3 and t[2] == 0 for t in st) or b >= 4  # (starts a and b: step 0 stalls at the entry)
        assert np.array_equal(a["el"][b, 1:], el0[1:]) and np.array_equal(a["el"][b, 0, [0, 2, 3]], el0[0, [0, 2, 3]])
        assert np.array_equal(a["el"][b, 0, [1, 4, 5]], h_run[0]) and np.array_equal(a["fin"][b, [2, 3, 5]], h_fin) and np.all(h_run[1:] != 0.0)
    assert e["brachi"]["el"].shape == (3, N, 0) and np.all(e["brachi"]["fin"][:, 0] == 0.0) and np.all(e["brachi"]["fin"][:, 1] != 0.0)
    h = e["brachi_hli"]["el"]  # (mu_li, last_hli)
    assert np.all(h[:, :, 0] == 1.0) and np.all(h[:, 0, 1] != 0.0) and np.all(h[:, 1:, 1] == 0.0)
    for tag in e:
        assert np.all(e[tag]["w"] == MC.ENTRY_W)


def test_gt_for_ge_at_zero_cannot_show(oracle_built):
    """the one mistake no case can catch, `>` in place of `>=`: where an inequality is exactly 0 the active form mu (2 h w + 1) and the
    inactive form mu / ((1 - h w) (1 - h w)) are the same bits, mu — in the update here, and in the penalty and its derivatives
    (iLQG_func.c:242-245, 312-315, 330-333: h mu (h w + 1) = h mu / (1 - h w) = 0, slopes mu, curvatures 2 mu w).  Asserted on
    the restatement of the update over every case, and on the penalty's own arithmetic at the zero cases, with +0.0 and -0.0"""
    o_rows = dict(tol=MC.TOL_DEFAULT, fact1=MC.FACT1_DEFAULT, max_l=np.inf, max_f=np.inf)
    tables = [(name, MC.reference(name), MC.options(name)) for name in NAMES] + [("rows", MC.rows_reference(), o_rows)]
    at_zero = 0
    for name, t, o in tables:  # the restatement with `>` switched on: no case of any batch or of the rows form differs
        for b in range(len(t["cls"])):
            args = (t["h_run"][b], t["h_fin"][b], t["el_in"][b], t["fin_in"][b], t["w_in"][b], o)
            assert not differs(update_np(*args), update_np(*args, mut="gt_for_ge")), (name, b, t["cls"][b])
            at_zero += int(np.any(t["h_run"][b, :, 1:] == 0.0) or t["h_fin"][b, 2] == 0.0)
    rows_cls = MC.rows_reference()["cls"]
    assert at_zero == sum(c == "zero_hli" for c in MC.reference("free")["cls"]) + sum(c in ("hfi_zero", "hli_zero") for c in rows_cls) >= 8  # (the switch does take the other form there)
    r = MC.reference("free")
    zero = [b for b, c in enumerate(r["cls"]) if c == "zero_hli"]
    assert len(zero) >= 2
    for b in zero:
        mu, w = r["el_in"][b, 0, 2], r["w_in"][b, 0]
        for h in (0.0, -0.0):
            assert mu * (2.0 * h * w + 1.0) == mu / ((-h * w + 1.0) * (-h * w + 1.0)) == mu == r["el"][b, 0, 2]
            assert h * mu * (h * w + 1.0) == h * mu / (-h * w + 1.0) == 0.0
            assert h * mu * w + mu * (h * w + 1.0) == h * mu * w / ((-h * w + 1.0) * (-h * w + 1.0)) + mu / (-h * w + 1.0) == mu
            assert 2.0 * mu * w == 2.0 * h * mu * (w * w) / ((-h * w + 1.0) ** 3) + 2.0 * mu * w / ((-h * w + 1.0) * (-h * w + 1.0))


@pytest.mark.parametrize("mut", UPDATE_MUTATIONS + INIT_MUTATIONS)
def test_every_mistake_in_the_update_is_caught_by_some_case(oracle_built, mut):
    caught = []
    if mut in INIT_MUTATIONS:
        o = dict(tol=MC.TOL_DEFAULT, fact1=MC.FACT1_DEFAULT, max_l=np.inf, max_f=np.inf)
        for b, ((h_run, h_fin), el0, fin0) in enumerate(entry_inputs()):
            if differs(update_np(h_run, h_fin, el0, fin0, MC.ENTRY_W, o, 1), update_np(h_run, h_fin, el0, fin0, MC.ENTRY_W, o, 1, mut)):
                caught.append(("entry", b, "entry"))
    else:
        for name in NAMES:
            r = MC.reference(name)
            for b, (good, bad) in enumerate(zip(restated(name), restated(name, mut))):
                if differs(good, bad):
                    caught.append((name, b, r["cls"][b]))
    print("%s: caught by %d cases, classes %s" % (mut, len(caught), sorted(set(c[2] for c in caught))))
    assert caught, mut


# ---------------------------------------------------------------------------
# step 4 restated on the driver's single stages (iLQG.c:224-379), with its mistakes
# ---------------------------------------------------------------------------
STEP4_MUTATIONS = ("no_raise_at_lambda_max_exit", "no_resweep_at_exit", "derivatives_follow_the_raise")
STD = dict(tolFun=1e-7, tolGrad=1e-5, lambdaInit=1.0, dlambdaInit=1.0, lambdaFactor=1.6, lambdaMax=1e10, lambdaMin=1e-6, w_pen_max_l=np.inf, w_pen_max_f=np.inf)


_solved = {}


def restated_solve(name, fd, max_iter, mut=None):
    """(cost, (w_pen_l, w_pen_f), lambda, iterations, rc, [(g_norm, dV0, dV1)] per line search); computed once per process"""
    key = (name, fd, max_iter, mut)
    if key not in _solved:
        _solved[key] = _restated_solve(name, fd, max_iter, mut)
    return _solved[key]


def _restated_solve(name, fd, max_iter, mut):
    opts = dict(MC.SEQ[name][0], max_iter=max_iter)
    o = dict(STD, **opts)
    d = Driver(lib_path("oracle", "almix", fd), MC.SEQ_N, MC.almix_params(MC.SEQ_N), opts)
    assert d.init(*MC.seq_start()) == 1
    lam, dl, need, done, it, trace = o["lambdaInit"], o["dlambdaInit"], True, False, 0, []

    def up(lam, dl):
        dl = max(dl * o["lambdaFactor"], o["lambdaFactor"])
        return max(lam * dl, o["lambdaMin"]), dl

    def down(lam, dl):
        dl = min(dl / o["lambdaFactor"], 1.0 / o["lambdaFactor"])
        return lam * dl * (lam > o["lambdaMin"]), dl
    while it < max_iter:
        if need:
            assert d.calc_derivs() == 1
            need = False
        done = False
        while not done:
            d.set_lambda(lam)
            if d.back_pass():
                lam, dl = up(lam, dl)
                if lam > o["lambdaMax"]:
                    break
            else:
                done = True
        sc = d.scalars()
        if sc["g_norm"] < o["tolGrad"] and lam < 1e-5:
            lam, dl = down(lam, dl)
            break
        if not done:
            break
        accepted = d.line_search(it)
        trace.append((sc["g_norm"], sc["dV0"], sc["dV1"]))
        if accepted:
            lam, dl = down(lam, dl)
            d.accept()
            need = True
            if d.scalars()["dcost"] < o["tolFun"]:
                break
            assert d.update_multipliers(0) == 1 and d.cost_resweep() == 1
        else:
            lam, dl = up(lam, dl)
            leaving = lam > o["lambdaMax"]
            if o["w_pen_fact2"] > 1.0 and not (leaving and mut == "no_raise_at_lambda_max_exit"):
                w = d.multipliers()[2]
                x, u = d.traj(0)
                d.set_state(x, u, d.scalars()["cost"], lam, (min(o["w_pen_max_l"], w[0] * o["w_pen_fact2"]), min(o["w_pen_max_f"], w[1] * o["w_pen_fact2"])))
                if not (leaving and mut == "no_resweep_at_exit"):
                    assert d.cost_resweep() == 1
                if mut == "derivatives_follow_the_raise":
                    need = True
            if leaving:
                break
        it += 1
    out = (d.scalars()["cost"], d.multipliers()[2], lam, it, int(done and it < max_iter), trace)
    d.close()
    return out


def sequence_differs(name, fd, mut):
    s = MC.sequence_reference(name, fd)
    for m in range(1, MC.SEQ[name][1] + 1):
        cost, w, lam, it, rc, trace = restated_solve(name, fd, m, mut)
        j = m - 1
        if (cost, w, lam, it, rc) != (s["cost"][j], tuple(s["w"][j]), s["lambda"][j], s["iterations"][j], s["rc"][j]):
            return True
    return [t[0] for t in trace] != list(s["trace_g_norm"]) or [t[1] for t in trace] != list(s["trace_dV0"]) or [t[2] for t in trace] != list(s["trace_dV1"])


@pytest.mark.parametrize("fd", [0, 1])
def test_sequences_are_what_their_labels_say(oracle_built, fd):
    S = {name: MC.sequence_reference(name, fd) for name in MC.SEQ}
    none = 9  # (eight step sizes by default: log_linesearch = n_alpha + 1 where nothing is accepted)
    for name in ("rej3", "rej3_caps", "rej_lambda_max", "rej_fact2_1", "rej_above_cap"):
        assert np.all(S[name]["trace_alpha_idx"] == 2) and np.all(S[name]["trace_bp_calls"] == 1), name  # alpha = [0.0]: every search rejected
        assert np.all(S[name]["el"][:, :, [0]] == 0.0) and np.all(S[name]["el"][:, :, 2:4] == 1.0), name  # no update has run
    A, FUN, MAXI, LMAX = MC.ST_ACTIVE, MC.ST_CONVERGED_FUN, MC.ST_MAX_ITER, MC.ST_LAMBDA_MAX
    want = dict(rej3=[A, A, MAXI], rej3_caps=[A, A, MAXI], rej_lambda_max=[A, A, A, LMAX, LMAX, LMAX], rej_fact2_1=[A, A, MAXI], rej_above_cap=[A, MAXI],
                tol_fun=[A, FUN, FUN], accepted=[A, A, MAXI])
    assert set(want) == set(MC.SEQ) and all(S[name]["status"].tolist() == want[name] for name in want), {name: S[name]["status"] for name in want}
    assert S["rej3"]["w"].tolist() == [[4, 4], [8, 8], [16, 16]] and S["rej3"]["iterations"].tolist() == [1, 2, 3] and not S["rej3"]["rc"].any()
    assert np.all(np.diff(np.concatenate([[S["rej3"]["init_cost"]], S["rej3"]["cost"]])) > 1.0)  # re-swept each time
    assert S["rej3_caps"]["w"].tolist() == [[4, 4], [8, 5], [10, 5]]
    lm = S["rej_lambda_max"]
    assert lm["w"].tolist()[2:] == [[16, 16], [32, 32], [32, 32], [32, 32]] and lm["iterations"].tolist() == [1, 2, 3, 3, 3, 3] and lm["rc"].tolist() == [0, 0, 0, 1, 1, 1]
    assert lm["lambda"][3] > 50.0 > lm["lambda"][2] and lm["cost"][3] > lm["cost"][2] + 1.0 and len(lm["trace_alpha_idx"]) == 4
    f1 = S["rej_fact2_1"]
    assert np.all(f1["w"] == 2.0) and np.all(f1["cost"] == f1["init_cost"])
    assert S["rej_above_cap"]["w"].tolist() == [[1, 1.5], [1, 1.5]]
    tf = S["tol_fun"]
    first = int(np.argmax(tf["trace_alpha_idx"] < none))  # the first accepted search
    assert tf["trace_alpha_idx"][first] < none and tf["rc"][first] == 1 and tf["iterations"][first] == first
    assert np.all(tf["el"][:, :, 0] == 0.0) and np.all(tf["fin"][:, :2] == 0.0) and np.all(tf["el"][:, :, 2:4] == 1.0)  # mu as init_multipliers() left them
    ac = S["accepted"]
    K = MC.SEQ["accepted"][1]
    assert ac["trace_alpha_idx"][K - 1] < none and ac["iterations"][K - 1] == K and ac["rc"][K - 1] == 0
    assert np.any(ac["fin"][K - 1, :2] != 0.0) and np.any(ac["w"][K - 1] != ac["w"][0])  # the update has run, and raised


@pytest.mark.parametrize("fd", [0, 1])
def test_restated_step_4_equals_the_reference(oracle_built, fd):
    for name in MC.SEQ:
        assert not sequence_differs(name, fd, None), name


@pytest.mark.parametrize("mut", STEP4_MUTATIONS)
def test_every_mistake_in_step_4_is_caught_by_some_sequence(oracle_built, mut):
    caught = [(name, fd) for name in MC.SEQ for fd in (0, 1) if sequence_differs(name, fd, mut)]
    print("%s: caught by %s" % (mut, caught))
    assert caught, mut
