"""TEST INFRASTRUCTURE — one generated table for the augmented-Lagrangian step of the solver: update_multipliers()
(iLQG_func.tem:419-521, problems/almix/iLQG_func.c:584-660) on every branch it separates, the entry form update_multipliers(o, 1)
of iLQG.c:237, and step 4 of the iteration (iLQG.c:311-361: accept / update / re-sweep, reject / raise by w_pen_fact2 /
re-sweep / lambdaMax exit) as sequences through the reference's own iLQG().  tests/test_multiplier_cases_recipe.py pins the
table to the reference build and to tests/golden/multipliers.npz (no GPU); tests/test_gpu_multiplier_branches.py uses it for
k_multipliers / multipliers_lane, k_multipliers_rows, the wave mapping's kernel, k_update and the cost-only roll-out.

SINGLE UPDATES.  almix, n_hor = 6: 3 states, 2 inputs, hle[1], hli[2], hfe[2], hfi[1], so multipliersEl_t is
(mu_le, last_hle, mu_li[2], last_hli[2]) and multipliersFin_t (mu_fe[2], last_hfe[2], mu_fi, last_hfi).  A case is ONE
trajectory: a start (x0, u0) rolled out by init(), so that (x, u) and the auxiliaries agree on the CPU (which reads the
auxiliaries its roll-out stored) and on the device (which recomputes them); the two weights; and multiplier structs whose
mu_* are all non-zero and whose last_h* are CHOSEN from the constraint values h the roll-out has:
    quiet (the default)   last = 2 max(fact1, 1) |h| (1 where h == 0): fact1 v > last is false
    ("hle", 0, k) ("hli", i, k) ("hfe", i) ("hfi", 0) in `stall`:   last = h / 2 — the violation grows
    `last` = {trigger: ratio}:   last = ratio h, whatever that makes of the test (negative values, the other sign)
The starts:  a  x0 = (0, 0.6, -0.3), a = (-1, -1, 0.5, 1, 1, -0.5), s = 0.3: hli_1 = v - tgt[2] is + + - - + + along the steps,
                hle_1 > 0 on steps 0 to 4 and < 0 on step 5, hli_2 < 0, hfe both > 0, hfi < 0
             b  the same with p and q moved by 1.5: the same velocities, and the final position beyond its bound, hfi > 0
             c  a mirrored (x0, u0 negated): v < 0, so hli_2 = -v - tgt[2] takes hli_1's pattern, hle_1 and both hfe < 0
A batch is a list of cases under ONE set of options (they are the solver's, not the trajectory's): `free` without caps,
`caps` with w_pen_max (10, 7), `tol2` with tolConstraint = 1e-2, `fact1` with w_pen_fact1 = 1 and the caps.  Classes are
interleaved (b % n_classes), so neighbouring lanes of a wavefront take different branches; every class has at least two cases;
no batch size is a multiple of 64.  `rnd` varies the start (by exact binary fractions) and the multipliers, not the branch.

Conditions (asserted by the recipe test on the reference's numbers): the stalls that happen are exactly those the case names;
no violation v lies within 1e-6 relative of tolConstraint and no fact1 v within 1e-6 relative of last, apart from the
deliberate zeros — so FMA contraction in the product builds (which can move an auxiliary by a last place) flips no decision.

THE ROWS FORM (ROWS): the trajectory of start a in every slot, each slot with its own tgt row and vref window: hfi = p_N -
tgt[1] exactly zero, just inside / outside the tolerance and beyond it, hli_1 of step 0 the same through tgt[2], hle through vref.

THE ENTRY FORM (ENTRY): what drv_init leaves — last_h* of step 0 only, steps 1.. as init_multipliers() left them, last_hf* of
the final part, no mu and no weight moved although step 0 stalls (last = 0 < fact1 v) — on almix, brachi (no running
constraint) and brachi_hli.

STEP-4 SEQUENCES (SEQ): almix, n_hor = 8, FULL_DDP 0 and 1, options only: alpha = [0.0] makes expected == 0 in every search,
so every iteration is rejected.  Run with max_iter = 1 .. K; recorded per max_iter: cost, both weights, lambda, iterations,
the return code, the multipliers, the trace of the longest run, and the status a device run holds after as many iterations.

What is NOT compared: nothing of update_multipliers() is left out.  One mistake cannot show in any case: `>` in place of `>=`
where an inequality is exactly 0 — the active form mu (2 h w + 1) and the inactive form mu / (1 - h w)^2 are both mu at h == 0,
bit for bit (the penalty is built twice continuously differentiable there); the recipe test asserts exactly that, on every case.
"""
import os

import numpy as np

from oracle.harness import Driver, brachi_hli_case, lib_path

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "multipliers.npz")
N = 6
TGT = (2.0, 1.55, 0.45)
MARGIN = 1e-6
TOL_DEFAULT, FACT1_DEFAULT = 1e-7, 4.0
NEAR = 2.0 ** -10  # "just" inside / outside the tolerance: a thousand times the margin


def almix_params(n, tgt=TGT, vref=None):
    return dict(h=[0.1], cu=[0.05, 0.02], cx=[0.3, 0.05, 0.02], cf=[4.0, 1.0, 2.0], lim=[-1.1, 1.1], tgt=list(tgt),
                vref=(0.8 + 0.4 * np.sin(np.arange(n + 1) * 0.2)) if vref is None else vref)


U_A = (-1.0, -1.0, 0.5, 1.0, 1.0, -0.5, 0.5, -1.0)  # (the first 6: the single updates; all 8: the sequences)
STARTS = {"a": ((0.0, 0.6, -0.3), 1.0), "b": ((1.5, 0.6, 1.2), 1.0), "c": ((0.0, -0.6, 0.3), -1.0)}


def start(name, rnd=0, n=N, v0=None):
    """(x0, u0) of a start; rnd moves the velocity and the towed position by exact binary fractions; v0 replaces the velocity"""
    x0, sign = STARTS[name]
    x0 = np.array(x0) + sign * rnd * np.array([0.0, 2.0 ** -8, 2.0 ** -9])
    if v0 is not None:
        x0[1] = v0
    u0 = np.zeros((n, 2))
    u0[:, 0], u0[:, 1] = sign * np.array(U_A[:n]), sign * 0.3
    return x0, u0


def case(st, w, stall=(), last=None, v0=None):
    return dict(start=st, w=w, stall=tuple(stall), last=dict(last or {}), v0=v0)


RUN0, RUN2, RUN5 = ("hle", 0, 0), ("hle", 0, 2), ("hli", 0, 5)
FIN = ("hfe", 0)


def _free_classes():
    tol = TOL_DEFAULT
    return {
        "none": [case("a", (3.0, 5.0)), case("b", (2.0, 0.5)), case("c", (1.5, 2.5))],
        "step_first": [case("a", (3.0, 5.0), [RUN0]), case("a", (2.0, 3.0), [("hli", 0, 0)]), case("c", (1.0, 2.0), [("hli", 1, 0)])],
        "step_middle": [case("a", (3.0, 5.0), [RUN2]), case("a", (0.5, 5.0), [("hli", 0, 1)]), case("c", (3.0, 1.0), [("hli", 1, 4)])],
        "step_last": [case("a", (3.0, 5.0), [RUN5]), case("a", (1.0, 1.0), [("hle", 0, 5)]), case("c", (2.0, 2.0), [("hli", 1, 5)])],
        "steps_several": [case("a", (3.0, 5.0), [RUN0, RUN2, RUN5]), case("a", (1.25, 5.0), [("hle", 0, 1), ("hli", 0, 4)])],
        "final_only": [case("a", (3.0, 5.0), [FIN]), case("b", (3.0, 2.0), [("hfi", 0)]), case("c", (3.0, 4.0), [("hfe", 1)])],
        "both_parts": [case("a", (3.0, 5.0), [RUN2, FIN]), case("b", (2.0, 1.0), [RUN5, ("hfi", 0), ("hfe", 1)]), case("c", (1.0, 3.0), [("hli", 1, 0), ("hfe", 0)])],
        # each constraint the only trigger in turn
        "only_hle0": [case("a", (3.0, 5.0), [("hle", 0, 3)]), case("c", (3.0, 5.0), [("hle", 0, 1)])],
        "only_hli0": [case("a", (3.0, 5.0), [("hli", 0, 4)]), case("b", (3.0, 5.0), [("hli", 0, 1)])],
        "only_hli1": [case("c", (3.0, 5.0), [("hli", 1, 1)]), case("c", (2.0, 5.0), [("hli", 1, 4)])],
        "only_hfe0": [case("a", (3.0, 5.0), [("hfe", 0)]), case("c", (3.0, 2.0), [("hfe", 0)])],
        "only_hfe1": [case("a", (3.0, 5.0), [("hfe", 1)]), case("c", (3.0, 2.0), [("hfe", 1)])],
        "only_hfi0": [case("b", (3.0, 5.0), [("hfi", 0)]), case("b", (1.0, 0.25), [("hfi", 0)])],
        # hli_1 of step 0 = x0[1] - tgt[2], violated and growing (last = h / 2), just inside and just outside the tolerance
        "tol_inside": [case("a", (3.0, 5.0), last={("hli", 0, 0): 0.5}, v0=TGT[2] + tol * (1 - NEAR)), case("b", (2.0, 5.0), last={("hli", 0, 0): 0.5}, v0=TGT[2] + tol * (1 - 4 * NEAR))],
        "tol_outside": [case("a", (3.0, 5.0), [("hli", 0, 0)], v0=TGT[2] + tol * (1 + NEAR)), case("b", (2.0, 5.0), [("hli", 0, 0)], v0=TGT[2] + tol * (1 + 4 * NEAR))],
        # an equality with a negative value stalls through fabs: last of the same sign, and of the other
        "eq_negative": [case("c", (3.0, 5.0), [("hle", 0, 2)]), case("c", (3.0, 5.0), [("hfe", 0)], last={("hfe", 0): -0.5}), case("a", (2.0, 5.0), [("hle", 0, 5)], last={("hle", 0, 5): -0.25})],
        # an inequality that is negative and grows in magnitude: no raise (the comparison is signed)
        "ineq_negative": [case("a", (3.0, 5.0), last={("hli", 1, 2): 0.5, ("hli", 0, 3): 0.5}), case("a", (3.0, 5.0), last={("hfi", 0): 0.5}), case("c", (3.0, 5.0), last={("hli", 0, 0): 0.25, ("hli", 0, 5): 0.5})],
        # hli_1 == 0.0 exactly at step 0: `>=` takes the active formula; not above the tolerance, so no stall whatever last is
        "zero_hli": [case("a", (3.0, 5.0), v0=TGT[2]), case("b", (2.0, 5.0), v0=TGT[2])],
    }


def _caps_classes():
    both = [RUN2, FIN]
    return {
        "uncapped": [case("a", (1.0, 1.5), both), case("b", (2.0, 0.5), both)],
        "l_capped_only": [case("a", (3.0, 1.0), both), case("c", (9.0, 1.5), both)],
        "f_capped_only": [case("a", (1.0, 5.0), both), case("c", (2.25, 2.0), both)],
        "both_capped": [case("a", (3.0, 5.0), both), case("b", (2.75, 6.5), both)],
        "at_cap": [case("a", (10.0, 7.0), both), case("a", (10.0, 1.0), [RUN0]), case("b", (1.0, 7.0), [("hfi", 0)])],
        # above the cap: down to the cap on a stall, untouched otherwise
        "above_cap_stall": [case("a", (15.0, 9.0), both), case("a", (15.0, 9.0), [RUN5]), case("b", (15.0, 9.0), [("hfe", 1)])],
        "above_cap_quiet": [case("a", (15.0, 9.0)), case("c", (11.0, 7.5))],
    }


def _tol2_classes():
    tol = 1e-2
    return {
        "tol_inside": [case("a", (3.0, 5.0), last={("hli", 0, 0): 0.5}, v0=TGT[2] + tol * (1 - NEAR)), case("b", (2.0, 5.0), last={("hli", 0, 0): 0.5}, v0=TGT[2] + tol * (1 - 4 * NEAR))],
        "tol_outside": [case("a", (3.0, 5.0), [("hli", 0, 0)], v0=TGT[2] + tol * (1 + NEAR)), case("b", (2.0, 5.0), [("hli", 0, 0)], v0=TGT[2] + tol * (1 + 4 * NEAR))],
        "none": [case("a", (3.0, 5.0)), case("c", (1.5, 2.5))],
        "both_parts": [case("a", (3.0, 5.0), [RUN2, FIN]), case("c", (1.0, 3.0), [("hli", 1, 0), ("hfe", 0)])],
    }


def _fact1_classes():
    """w_pen_fact1 = 1: a stall multiplies by 1 — nothing moves but a weight above its cap"""
    return {
        "f1_stall": [case("a", (3.0, 5.0), [RUN2, FIN]), case("c", (1.0, 3.0), [("hli", 1, 0), ("hfe", 0)])],
        "f1_none": [case("a", (3.0, 5.0)), case("a", (15.0, 9.0))],
        "f1_above_cap": [case("a", (15.0, 9.0), [RUN2, FIN]), case("b", (15.0, 2.0), [RUN0])],
    }


COMMON = dict(w_pen_fact2=2.0, max_iter=5)
CAPS = dict(w_pen_max_l=10.0, w_pen_max_f=7.0)
# name: (options, classes, trajectories)
BATCHES = {
    "free": (dict(COMMON), _free_classes(), 130),  # two wavefronts and two lanes of a third
    "caps": (dict(COMMON, **CAPS), _caps_classes(), 37),
    "tol2": (dict(COMMON, tolConstraint=1e-2), _tol2_classes(), 13),
    "fact1": (dict(COMMON, w_pen_fact1=1.0, **CAPS), _fact1_classes(), 11),
}
EL = dict(mu_le=(0,), last_hle=(1,), mu_li=(2, 3), last_hli=(4, 5))
FI = dict(mu_fe=(0, 1), last_hfe=(2, 3), mu_fi=(4,), last_hfi=(5,))
RUNNING = (("hle", 0, "e", 0, 1), ("hli", 0, "i", 2, 4), ("hli", 1, "i", 3, 5))  # kind, index, eq / ineq, column of mu, column of last
FINAL = (("hfe", 0, "e", 0, 2), ("hfe", 1, "e", 1, 3), ("hfi", 0, "i", 4, 5))


def options(name):
    o = BATCHES[name][0]
    return dict(tol=o.get("tolConstraint", TOL_DEFAULT), fact1=o.get("w_pen_fact1", FACT1_DEFAULT), fact2=o["w_pen_fact2"],
                max_l=o.get("w_pen_max_l", np.inf), max_f=o.get("w_pen_max_f", np.inf))


def specs(name):
    """[(class, case, round)] of batch `name`, classes interleaved"""
    classes = BATCHES[name][1]
    names = list(classes)
    out = []
    for b in range(BATCHES[name][2]):
        cls, r = names[b % len(names)], b // len(names)
        out.append((cls, classes[cls][r % len(classes[cls])], r // len(classes[cls])))
    return out


def values(kind, fd, params, opts, x0, u0, problem="almix", cols=((1, 4, 5), (2, 3, 5))):
    """(h_run [n, ME / 2], h_fin [MF / 2], x, u, cost) of a start: the constraint values of its roll-out, read as the last_h*
    an update leaves (cols: the columns of last_h* in the two structs)"""
    d = Driver(lib_path(kind, problem, fd), len(u0), params, opts)
    assert d.init(x0, u0) == 1
    x, u = d.traj(0)
    cost = d.scalars()["cost"]
    assert d.update_multipliers(0) == 1
    el, fin, _ = d.multipliers()
    d.close()
    return el[:, list(cols[0])], fin[list(cols[1])], x, u, cost


def structs(c, h_run, h_fin, fact1, seed):
    """the multiplier structs a case enters the update with: every mu non-zero (mu_li, mu_fi positive, as the updates keep
    them), last_h* by the case's rules"""
    rng = np.random.default_rng(seed)
    n = len(h_run)
    el, fin = np.zeros((n, 6)), np.zeros(6)
    el[:, 0] = rng.uniform(0.1, 0.5, n) * rng.choice([-1.0, 1.0], n)
    el[:, 2:4] = rng.uniform(0.5, 1.5, (n, 2))
    fin[0:2] = rng.uniform(0.1, 0.5, 2) * rng.choice([-1.0, 1.0], 2)
    fin[4] = rng.uniform(0.5, 1.5)

    def last_of(trig, h):
        if trig in c["last"]:
            return c["last"][trig] * h
        if trig in c["stall"]:
            return 0.5 * h
        return 2.0 * max(fact1, 1.0) * abs(h) if h != 0.0 else 1.0
    for j, (kind, i, _, _, col) in enumerate(RUNNING):
        for k in range(n):
            el[k, col] = last_of((kind, i, k), h_run[k, j])
    for j, (kind, i, _, _, col) in enumerate(FINAL):
        fin[col] = last_of((kind, i), h_fin[j])
    return el, fin


_built = {}
FIELDS = ("x0", "u0", "x", "u", "h_run", "h_fin", "el_in", "fin_in", "w_in", "cost_in", "new_cost", "el", "fin", "w", "cost", "w_rej", "cost_rej")


def one_update(kind, problem, fd, params, opts, o, x0, u0, x, u, el_in, fin_in, w_in, cost_in, new_cost):
    """one case on the driver build `kind`: dict of everything FIELDS names behind the inputs — what update_multipliers(o, 0)
    and the re-sweep leave from (el_in, fin_in, w_in, new_cost) (el fin w cost: iLQG.c:337-338), and what a rejected step
    leaves (w_rej = min(max, w fact2), cost_rej re-swept under them with el_in / fin_in: iLQG.c:345-349)"""
    d = Driver(lib_path(kind, problem, fd), len(u0), params, opts)
    assert d.init(x0, u0) == 1
    d.set_multipliers(el_in, fin_in)
    d.set_state(x, u, new_cost, 1.0, w_in)
    assert d.update_multipliers(0) == 1 and d.cost_resweep() == 1
    el, fin, w = d.multipliers()
    cost = d.scalars()["cost"]
    w_rej = (min(o["max_l"], w_in[0] * o["fact2"]), min(o["max_f"], w_in[1] * o["fact2"]))
    d.set_multipliers(el_in, fin_in)
    d.set_state(x, u, cost_in, 1.0, w_rej)
    assert d.cost_resweep() == 1
    cost_rej = d.scalars()["cost"]
    d.close()
    return dict(x0=x0, u0=u0, x=x, u=u, el_in=el_in, fin_in=fin_in, w_in=w_in, cost_in=cost_in, new_cost=new_cost, el=el, fin=fin, w=w, cost=cost,
                w_rej=w_rej, cost_rej=cost_rej)


def collect(rows, **extra):
    """the cases' dicts as arrays over the batch, with the lists of `extra` beside them"""
    out = {k: np.array([r[k] for r in rows], dtype=np.float64) for k in rows[0]}
    out.update(extra)
    return out


def reference(name, kind="oracle", fd=0):
    """everything about batch `name` from the driver build `kind`, once per process: per trajectory the inputs (x0 u0, the
    rolled-out x u, h_run h_fin, el_in fin_in w_in, cost_in = the roll-out's cost under zero weights, new_cost = what an
    accepted search would have left) and the results of one_update(); cls, case: the class names and case dicts"""
    key = (name, kind, fd)
    if key in _built:
        return _built[key]
    opts, o = BATCHES[name][0], options(name)
    params = almix_params(N)
    rows, cls, cases = [], [], []
    for b, (c_name, c, rnd) in enumerate(specs(name)):
        x0, u0 = start(c["start"], rnd, N, c["v0"])
        h_run, h_fin, x, u, cost_in = values(kind, fd, params, opts, x0, u0)
        el_in, fin_in = structs(c, h_run, h_fin, o["fact1"], 1000 * (1 + list(BATCHES).index(name)) + b)
        rows.append(dict(one_update(kind, "almix", fd, params, opts, o, x0, u0, x, u, el_in, fin_in, c["w"], cost_in, cost_in + 0.25 * (b + 1)), h_run=h_run, h_fin=h_fin))
        cls.append(c_name)
        cases.append(c)
    _built[key] = collect(rows, cls=cls, case=cases)
    return _built[key]


# ---------------------------------------------------------------------------
# brachi_hli (the problem the wave mapping is built for): one running inequality, one final equality
# ---------------------------------------------------------------------------
HLI_B = 11
HLI_OPTS = dict(COMMON, w_pen_max_l=100.0)
HLI_CLASSES = ("none", "run_first", "fin", "both", "neg_growing", "run_last")
HLI_Y0 = ((-1e-3, 1.0), (-0.5, 1.5), (-0.75, 1.25))  # (y0, slope): the first stays above ymin (hli < 0), the others fall below it from step 1 on


def hli_reference(kind="oracle"):
    """reference() for brachi_hli at n_hor = 6: multipliersEl_t (mu_li, last_hli), multipliersFin_t (mu_fe, last_hfe); hli =
    ymin - y, hfe = y_N - ymin_N.  Per class: nothing stalls; the first / the last step below ymin stalls; the final part; both;
    hli negative and growing in magnitude on every step (start 0: no raise)"""
    key = ("hli", kind)
    if key in _built:
        return _built[key]
    params = brachi_hli_case(N)[0]
    o = dict(tol=TOL_DEFAULT, fact1=FACT1_DEFAULT, fact2=HLI_OPTS["w_pen_fact2"], max_l=HLI_OPTS["w_pen_max_l"], max_f=np.inf)
    rows, cls, stalls = [], [], []
    for b in range(HLI_B):
        c_name = HLI_CLASSES[b % len(HLI_CLASSES)]
        y0, slope = HLI_Y0[0] if c_name in ("neg_growing", "none") and b % 2 == 0 else HLI_Y0[1 + b % 2]
        x0, u0 = np.array([y0 - 2.0 ** -6 * (b // len(HLI_CLASSES))]), -slope * np.ones((N, 1))
        h_run, h_fin, x, u, cost_in = values(kind, 0, params, HLI_OPTS, x0, u0, "brachi_hli", ((1,), (1,)))
        pos = np.flatnonzero(h_run[:, 0] > 0)
        steps = {"run_first": pos[:1], "run_last": pos[-1:], "both": pos[1:3]}.get(c_name, pos[:0])
        rng = np.random.default_rng(9000 + b)
        w_in = (40.0 / (1 + b), 0.5 * (1 + b))
        el_in, fin_in = np.zeros((N, 2)), np.zeros(2)
        el_in[:, 0], fin_in[0] = rng.uniform(0.5, 1.5, N), rng.uniform(0.1, 0.5)
        el_in[:, 1] = 2.0 * FACT1_DEFAULT * np.abs(h_run[:, 0])
        el_in[steps, 1] = 0.5 * h_run[steps, 0]
        if c_name == "neg_growing":
            neg = h_run[:, 0] < 0
            el_in[neg, 1] = 0.5 * h_run[neg, 0]
        fin_in[1] = (0.5 if c_name in ("fin", "both") else 2.0 * FACT1_DEFAULT) * h_fin[0]
        rows.append(dict(one_update(kind, "brachi_hli", 0, params, HLI_OPTS, o, x0, u0, x, u, el_in, fin_in, w_in, cost_in, cost_in + 0.25 * (b + 1)), h_run=h_run, h_fin=h_fin))
        cls.append(c_name)
        stalls.append((len(steps) > 0, c_name in ("fin", "both")))
    _built[key] = collect(rows, cls=cls, stalls=stalls)
    return _built[key]


# ---------------------------------------------------------------------------
# the rows form: one trajectory, a tgt row and a vref window per slot
# ---------------------------------------------------------------------------
ROWS_W = (3.0, 5.0)
ROWS_OPTS = dict(COMMON)


def rows_table(p_n, v_0):
    """[(class, tgt row, scale of the vref window)] from the final position p_N and the first velocity of start a's roll-out;
    slot 0 is the nominal row.  hfi = p_N - tgt[1]; hli_1 of step 0 = v_0 - tgt[2]; hle = s - vref v / 2"""
    tol = TOL_DEFAULT
    t = []
    t.append(("nominal", TGT, 1.0))
    t.append(("hfi_zero", (TGT[0], p_n, TGT[2]), 1.0))
    t.append(("hfi_inside", (TGT[0], p_n - tol * (1 - NEAR), TGT[2]), 1.0))
    t.append(("hfi_outside", (TGT[0], p_n - tol * (1 + NEAR), TGT[2]), 1.0))
    t.append(("hfi_beyond", (TGT[0], p_n - 0.25, TGT[2]), 1.0))
    t.append(("hfi_negative", (TGT[0], p_n + 0.25, TGT[2]), 1.0))
    t.append(("hli_zero", (TGT[0], TGT[1], v_0), 1.0))
    t.append(("hli_inside", (TGT[0], TGT[1], v_0 - tol * (1 - NEAR)), 1.0))
    t.append(("hli_outside", (TGT[0], TGT[1], v_0 - tol * (1 + NEAR)), 1.0))
    t.append(("hli_negative", (TGT[0], TGT[1], v_0 + 0.5), 1.0))
    t.append(("vref_high", TGT, 2.0))   # hle < 0 on every step
    t.append(("vref_low", TGT, 0.25))   # hle > 0 on every step
    t.append(("cost_only", (2.5, TGT[1], TGT[2]), 1.0))  # tgt[0] is in the final cost alone: the same update, another re-swept cost
    return t


def rows_growing(c_name):
    """the constraints of a slot whose remembered value is half the present one (a growing violation): the one the slot's row
    moves; every other is quiet, so the slot stalls exactly where its own row puts that constraint beyond the tolerance"""
    if c_name.startswith("hfi"):
        return {("hfi", 0): 0.5}
    if c_name.startswith("hli"):
        return {("hli", 0, 0): 0.5}
    if c_name.startswith("vref"):
        return {("hle", 0, k): 0.5 for k in range(N)}
    return {}


ROWS_B = 29  # the table, walked round: slots 13 .. 28 repeat it with other weights (no multiple of the table's length)


def rows_reference(kind="oracle", fd=0):
    """reference() for the rows batch, with tgt [B, 3] and vref [B, N + 1] beside: every slot on a Driver under that slot's own
    parameters; last_h* by rows_growing()"""
    key = ("rows", kind, fd)
    if key in _built:
        return _built[key]
    x0, u0 = start("a")
    _, _, x, u, _ = values(kind, fd, almix_params(N), ROWS_OPTS, x0, u0)
    table = rows_table(x[N, 0], x[0, 1])
    o = dict(fact2=ROWS_OPTS["w_pen_fact2"], max_l=np.inf, max_f=np.inf)
    rows, cls = [], []
    for b in range(ROWS_B):
        c_name, tgt, scale = table[b % len(table)]
        w_in = (ROWS_W[0] / (1 + b // len(table)), ROWS_W[1] * (1 + b // len(table)))
        params = almix_params(N, tgt, scale * almix_params(N)["vref"])
        h_run, h_fin, x_b, u_b, cost_in = values(kind, fd, params, ROWS_OPTS, x0, u0)
        assert np.array_equal(x_b, x) and np.array_equal(u_b, u)  # (no parameter of a row is in the dynamics)
        c = case("a", w_in, last=rows_growing(c_name))
        el_in, fin_in = structs(c, h_run, h_fin, FACT1_DEFAULT, 7000 + b)
        rows.append(dict(one_update(kind, "almix", fd, params, ROWS_OPTS, o, x0, u0, x, u, el_in, fin_in, w_in, cost_in, cost_in + 0.5 * (b + 1)),
                         h_run=h_run, h_fin=h_fin, tgt=tgt, vref=params["vref"]))
        cls.append(c_name)
    _built[key] = collect(rows, cls=cls)
    return _built[key]


# ---------------------------------------------------------------------------
# the entry form
# ---------------------------------------------------------------------------
BRACHI6 = dict(g=[9.81], yf=[-4.0], dx=[2 * np.pi / N])
ENTRY_W = (3.0, 5.0)


def entry_cases():
    """[(tag, problem, params, options, x0 [B, nx], u0 [B, N, nu])]: almix from its three starts (two rounds each), brachi and
    brachi_hli at n_hor = 6 from three starts each"""
    w = dict(w_pen_init_l=ENTRY_W[0], w_pen_init_f=ENTRY_W[1])
    al = [start(s, r) for s in "abc" for r in (0, 1)]
    hp, ho, hx0, hu0 = brachi_hli_case(N)
    y0 = np.array([[-1e-3], [-0.25], [-0.5]])
    slopes = -np.ones((3, N, 1)) * np.array([1.0, 0.5, 1.5])[:, None, None]
    return [("almix", "almix", almix_params(N), dict(COMMON, **w), np.array([a[0] for a in al]), np.array([a[1] for a in al])),
            ("brachi", "brachi", BRACHI6, dict(COMMON, **w), y0, slopes),
            ("brachi_hli", "brachi_hli", hp, dict(ho, **w), y0, slopes)]


def entry_reference(kind="oracle"):
    """{tag: dict(el [B, N, ME], fin [B, MF], w [B, 2], cost [B])} as drv_init leaves them"""
    key = ("entry", kind)
    if key in _built:
        return _built[key]
    out = {}
    for tag, problem, params, opts, x0, u0 in entry_cases():
        r = dict(el=[], fin=[], w=[], cost=[])
        for b in range(len(x0)):
            d = Driver(lib_path(kind, problem, 0), N, params, opts)
            assert d.init(x0[b], u0[b]) == 1
            el, fin, w = d.multipliers()
            r["el"].append(el), r["fin"].append(fin), r["w"].append(w), r["cost"].append(d.scalars()["cost"])
            d.close()
        out[tag] = {k: np.array(v, dtype=np.float64) for k, v in r.items()}
    _built[key] = out
    return out


# ---------------------------------------------------------------------------
# step 4 as sequences through iLQG()
# ---------------------------------------------------------------------------
SEQ_N = 8
SEQ_BASE = dict(w_pen_init_l=2.0, w_pen_init_f=2.0, w_pen_fact2=2.0)
REJECT = dict(SEQ_BASE, alpha=[0.0])
# name: (options without max_iter, K: run with max_iter = 1 .. K)
SEQ = {
    "rej3": (dict(REJECT), 3),                                            # weights 2, 4, 8, 16; the cost re-swept each time
    "rej3_caps": (dict(REJECT, w_pen_max_l=10.0, w_pen_max_f=5.0), 3),    # ends at (10, 5): a fact2 raise that lands on a cap
    "rej_lambda_max": (dict(REJECT, lambdaMax=50.0), 6),                  # leaves on the lambdaMax exit, weights raised and cost re-swept first
    "rej_fact2_1": (dict(REJECT, w_pen_fact2=1.0), 3),                    # no weight moves, the cost stays the initial cost's bits
    "rej_above_cap": (dict(REJECT, w_pen_max_l=1.0, w_pen_max_f=1.5), 2),  # the weights start above their caps: down on the first raise
    "tol_fun": (dict(SEQ_BASE, tolFun=1e9), 3),                           # leaves on the first accepted iteration, no multiplier update
    "accepted": (dict(SEQ_BASE), 3),                                      # max_iter reached on an accepted iteration: update and re-sweep have run
}
SEQ_SCALARS = ("cost", "lambda", "iterations")
ST_ACTIVE, ST_CONVERGED_FUN, ST_MAX_ITER, ST_LAMBDA_MAX = 0, 2, 3, 5  # ILQG_ST_* of ilqg_shim.h
TRACE = ("lambda", "g_norm", "dV0", "dV1", "cost", "new_cost", "alpha_idx", "bp_calls")


def seq_start():
    return start("a", 0, SEQ_N)


def sequence_reference(name, fd, kind="oracle"):
    """dict over max_iter = 1 .. K (index j = max_iter - 1): cost lambda iterations [K], w [K, 2], rc [K], el [K, N, 6], fin [K, 6],
    init_cost, the trace of the run with max_iter = K (one entry per line search), and status [K]: the ILQG_ST_* a device run
    with max_iter = K holds after j + 1 iterations, as the reference's runs imply it — no exit within max_iter = j + 1 (iterations
    == j + 1): ST_ACTIVE, or ST_MAX_ITER at j + 1 == K; an exit (iterations < j + 1, return code 1) behind search number
    `iterations` of the trace: ST_CONVERGED_FUN where that search accepted, ST_LAMBDA_MAX where it rejected"""
    key = ("seq", name, fd, kind)
    if key in _built:
        return _built[key]
    opts, K = SEQ[name]
    x0, u0 = seq_start()
    out = {k: [] for k in SEQ_SCALARS + ("w", "rc", "el", "fin")}
    for m in range(1, K + 1):
        d = Driver(lib_path(kind, "almix", fd), SEQ_N, almix_params(SEQ_N), dict(opts, max_iter=m))
        assert d.init(x0, u0) == 1
        if m == 1:
            init_cost = d.scalars()["cost"]
        rc = d.solve()
        sc = d.scalars()
        el, fin, w = d.multipliers()
        for k in SEQ_SCALARS:
            out[k].append(sc[k])
        out["w"].append(w), out["rc"].append(rc), out["el"].append(el), out["fin"].append(fin)
        trace = d.trace()
        d.close()
    out = {k: np.array(v, dtype=np.float64) for k, v in out.items()}
    out["init_cost"] = init_cost
    for k in TRACE:
        out["trace_" + k] = np.asarray(trace[k], dtype=np.float64)
    none = len(opts.get("alpha", range(8))) + 1  # (log_linesearch where nothing was accepted)
    status = []
    for j in range(K):
        it = int(out["iterations"][j])
        if it == j + 1:
            assert out["rc"][j] == 0
            status.append(ST_MAX_ITER if j + 1 == K else ST_ACTIVE)
        else:  # (no sequence leaves in a backward pass: the search the exit follows is in the trace)
            assert out["rc"][j] == 1 and it < len(trace["alpha_idx"])
            status.append(ST_CONVERGED_FUN if trace["alpha_idx"][it] < none else ST_LAMBDA_MAX)
    out["status"] = np.array(status, dtype=np.float64)
    _built[key] = out
    return out


def golden_of(kind="ref"):
    """what tests/golden/multipliers.npz records (tests/golden/make_goldens.py multipliers): results only"""
    out = {}
    for name in BATCHES:
        r = reference(name, kind)
        for k in ("h_run", "h_fin", "el", "fin", "w", "cost", "w_rej", "cost_rej"):
            out[name + "/" + k] = r[k]
    r = rows_reference(kind)
    for k in ("h_run", "h_fin", "el", "fin", "w", "cost"):
        out["rows/" + k] = r[k]
    r = hli_reference(kind)
    for k in ("h_run", "h_fin", "el", "fin", "w", "cost", "w_rej", "cost_rej"):
        out["hli/" + k] = r[k]
    for tag, r in entry_reference(kind).items():
        for k, v in r.items():
            out["entry_" + tag + "/" + k] = v
    for name in SEQ:
        for fd in (0, 1):
            for k, v in sequence_reference(name, fd, kind).items():
                out["seq_%s_fd%d/%s" % (name, fd, k)] = np.asarray(v)
    return out
