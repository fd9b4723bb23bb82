"""TEST INFRASTRUCTURE — one generated table of line searches that reach every branch line_search.c:37-75 separates, for
every device restatement of that scan: k_search (both stages, records through LDS or per lane, shared parameters or rows),
k_rollout + k_select (ls_keep 1 and 0) and the wave mapping's forms.  tests/test_linesearch_cases_recipe.py pins the
table to the reference build and to tests/golden/linesearch.npz (no GPU); tests/test_gpu_linesearch_branches.py uses it.

A case is ONE trajectory: a start (x0, u0 = 0), gains (l, L) and the three scalars the scan reads (cost, dV0, dV1); a
batch is a list of cases with one horizon, one list of step sizes and one zMin.  The gains decide which roll-outs fail,
the scalars decide which finite one is accepted:

  CarParking (FULL_DDP = 0) with d = 0.5, h = 0.03 and v = 40: the auxiliary s takes sqrt(d^2 - (h v sin w)^2), NaN once
  |h v sin w| > d, i.e. once the steering |w| > 0.43 (it is clamped to 0.5).
    ("one", k, lw)      l[k][0] = lw, everything else 0: w = alpha lw at step k — the step sizes with alpha lw > 0.43 fail,
                        a PREFIX of the (decreasing) list: lw 0.2 none, 0.5 one, 3.2 three, 1e3 all eight
    ("fb", l0, c, K)    l[0][0] = l0 <= 0.4 (finite at every alpha), l[1][0] = -c and a feedback K from the heading t to w at
                        step 1: w1 = -c alpha + K (t1(alpha) - t1(0)) is not monotonic in alpha — finite at alpha[0],
                        beyond the limit at alpha[1], finite from alpha[2] on: a failure BEHIND a finite roll-out
  brachi (one state, multipliers): the running cost takes sqrt(-y - dy dx); l[k][0] = lw > 0 turns the slope dy = -1 + alpha lw
  upwards, and from y0 = -0.5 the first one (lw = 2) or two (lw = 5) step sizes fail.  So brachi does give failures that
  depend on the step size, with wide margins.  Its roll-out costs RISE along the list (the nominal is the costliest), so
  only the first finite step size can be accepted: classes prefix-then-accept, all rejected, accepted at 0.

  With dV = (-1, 0) the expected reduction is alpha itself, and
    ("first", j)        cost halfway between c[j] and the lowest finite c[i], i < j: j is the first index with dcost > 0
    ("none",)           cost below every roll-out's: dcost < 0 everywhere, nothing accepted
    ("z", j, z)         cost = c[j] + z alpha[j] (the batch with zMin = 0.5)
    ("tie", j)          the cost next to c[j] + 0.5 alpha[j] at which the reference build's z is 0.5 EXACTLY: not > zMin,
                        rejected, and j + 1 accepted (searched over last-place neighbours; compared in FMA-free builds only)
  and with other dV
    ("neg", t)          dV = (1, -1 / sqrt(alpha[t] alpha[t+1])): expected > 0 up to index t and < 0 behind it, cost below
                        every roll-out's: the reference rejects all (z = 0 where expected <= 0); a scan without that guard
                        accepts at t + 1
    ("zero",)           dV = (0, 0), cost above every roll-out's: expected == 0 exactly with dcost > 0 — z = 0, not > zMin = 0

What is NOT compared (see reference()): new_cost after a scan whose last tried step size failed — the reference's
forward_pass returns at the failing callback with the partial sum, the device sums every step — and, for the same
reason, alpha_cost of a failed step size; dcost / expected where no step size tried has succeeded — uninitialised locals
of the reference's line_search(); the device keeps what the fields held (k_select's header comment), which the GPU tests
check with sentinels.

Conditions (asserted by the recipe test on the reference's numbers): every compared z at least 1e-6 max(1, |z|) from zMin
and every negative expected reduction at least 1e-6 from 0, apart from the one deliberate tie; every failing roll-out
fails at least 1 % beyond its limit and every finite one stays at least 1 % inside (margins()); every class has at least
two cases.
"""
import os

import numpy as np

from oracle.harness import CAR_PARAMS, Driver, lib_path

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "linesearch.npz")
CAR = dict(CAR_PARAMS, d=[0.5], h=[0.03])
CAR_X0 = (1.0, 1.0, 0.3, 40.0)
BRACHI = dict(g=[9.81], yf=[-4.0], dx=[2 * np.pi / 6])
BRACHI_OPTS = dict(w_pen_init_l=40.0, w_pen_init_f=40.0, w_pen_fact2=2.0)
ALPHA8 = 10.0 ** np.linspace(0.0, -3.0, 8)
Z_MARGIN = 1e-6
SENTINEL = dict(dcost=-777.25, expected=-555.5)  # what the device's fields hold before a search (set through set_scalar)

FB = (("fb", 0.4, 7.5, 6.0), ("fb", 0.4, 10.0, 8.0))  # ok pattern 1 0 1 1 1 1 1 1 at the horizons 2, 3 and 6


def _car_classes(n, k, k2):
    """{class: [(gains, scalars), ...]} for CarParking over ALPHA8 with zMin = 0; the large l sits on step k (k2: the other
    step used, so that both appear)"""
    free, p1, p3, dead = ("one", k, 0.2), ("one", k, 0.5), ("one", k2, 3.2), ("one", k, 1e3)
    return {
        "accept0": [(free, ("first", 0)), (("one", k2, 0.3), ("first", 0)), (FB[0], ("first", 0))],
        # every later index: the last of a first stage and the first of a second one for ls_split 1, 3, 4, and the last step size
        "accept_later": [(free if j % 2 else ("one", k2, 0.3), ("first", j)) for j in range(1, 8)],
        # right behind the prefix, or several step sizes later with finite rejected ones between; prefixes of 1 and 3 lie
        # inside a first stage, fill it (ls_split 3) or span the boundary (ls_split 1)
        "prefix_accept": [(p1, ("first", 1)), (p1, ("first", 4)), (p3, ("first", 3)), (p3, ("first", 4)), (p3, ("first", 6)),
                          (("one", k, 0.8), ("first", 2)), (("one", k2, 3.4), ("first", 7))],
        # alpha[0] finite and rejected, alpha[1] failed (dcost / expected stay alpha[0]'s), then accepted
        "fail_behind_finite": [(FB[0], ("first", 2)), (FB[1], ("first", 3)), (FB[1], ("first", 2))],
        "all_fail": [(dead, ("none",)), (("one", k2, 2e3), ("first", 0))],
        "neg_expected": [(free, ("neg", 0)), (free, ("neg", 3)), (p1, ("neg", 2)), (p3, ("neg", 5)), (FB[0], ("neg", 1))],
        "zero_expected": [(free, ("zero",)), (p1, ("zero",)), (FB[1], ("zero",))],
        "all_rejected": [(free, ("none",)), (("one", k2, 0.3), ("none",)), (p3, ("none",)), (FB[0], ("none",))],
    }


def _zmin_classes(n, k, k2):
    free, p1 = ("one", k, 0.2), ("one", k2, 0.5)
    return {
        "z_above": [(free, ("z", 0, 2.0)), (free, ("z", 3, 2.0)), (p1, ("z", 1, 2.0)), (free, ("z", 7, 0.75))],
        "z_below": [(free, ("z", 7, 0.3)), (p1, ("z", 7, 0.25)), (("one", k, 0.3), ("z", 7, 0.1))],
        "z_tie": [(free, ("tie", 0))],
        "all_fail": [(("one", k, 1e3), ("none",)), (("one", k2, 2e3), ("none",))],
    }


def _short_classes(n_alpha):
    """the second lists of step sizes: the first 4, 2, 1 of ALPHA8 (a search without a second stage at the default
    ls_split; T = 16, 32, 64 trajectories to a wavefront of k_search)"""
    free, p1, dead = ("one", 2, 0.2), ("one", 2, 0.5), ("one", 1, 1e3)
    out = {
        "accept0": [(free, ("first", 0)), (("one", 1, 0.3), ("first", 0))],
        "all_rejected": [(free, ("none",)), (("one", 1, 0.3), ("none",))],
        "all_fail": [(dead, ("none",)), (("one", 2, 2e3), ("first", 0))],
        "zero_expected": [(free, ("zero",)), (("one", 1, 0.3), ("zero",))],
    }
    if n_alpha >= 2:
        out["accept_later"] = [(free, ("first", n_alpha - 1)), (("one", 1, 0.3), ("first", 1))]
        out["prefix_accept"] = [(p1, ("first", 1)), (("one", 1, 0.8), ("first", n_alpha - 1))]
        out["neg_expected"] = [(free, ("neg", 0)), (p1, ("neg", 0))]
    if n_alpha == 2:
        # the scan ENDS on a failed step size behind a finite rejected one: dcost / expected are alpha[0]'s, new_cost is not compared
        out["end_on_failed"] = [(FB[0], ("none",)), (FB[1], ("none",)), (FB[0], ("zero",))]
    if n_alpha == 4:
        out["fail_behind_finite"] = [(FB[0], ("first", 2)), (FB[1], ("first", 3))]
    return out


def _brachi_classes():
    return {
        "accept0": [(("one", 0, 0.5), ("first", 0)), (("one", 2, 0.5), ("first", 0))],
        "prefix_accept": [(("one", 0, 2.0), ("first", 1)), (("one", 0, 5.0), ("first", 2)), (("one", 2, 5.0), ("first", 1))],
        "all_rejected": [(("one", 0, 0.5), ("none",)), (("one", 0, 5.0), ("none",)), (("one", 2, 5.0), ("zero",))],
    }


# name: (problem, n_hor, step sizes, zMin, classes, trajectories — the classes' cases in turn, b % n_classes, each class
# walking round its own list, the start varied with the round)
BATCHES = {
    "car6": ("carparking", 6, ALPHA8, 0.0, _car_classes(6, 2, 4), 200),  # (200: four stream groups of 64)
    "car2": ("carparking", 2, ALPHA8, 0.0, _car_classes(2, 0, 1), 56),
    "car3": ("carparking", 3, ALPHA8, 0.0, _car_classes(3, 1, 0), 56),
    "car6z": ("carparking", 6, ALPHA8, 0.5, _zmin_classes(6, 2, 3), 37),
    "car6a4": ("carparking", 6, ALPHA8[:4], 0.0, _short_classes(4), 37),
    "car6a2": ("carparking", 6, ALPHA8[:2], 0.0, _short_classes(2), 37),
    "car6a1": ("carparking", 6, ALPHA8[:1], 0.0, _short_classes(1), 70),
    "brachi6": ("brachi", 6, ALPHA8, 0.0, _brachi_classes(), 37),
}


def specs(name):
    """[(class, gains, scalars, round)] of batch `name`, classes interleaved"""
    classes = BATCHES[name][4]
    names = list(classes)
    out = []
    for b in range(BATCHES[name][5]):
        cls, r = names[b % len(names)], b // len(names)
        gains, scal = classes[cls][r % len(classes[cls])]
        out.append((cls, gains, scal, r // len(classes[cls])))
    return out


def setup(name):
    """(problem, n_hor, params, opts) of the batch's drivers and solvers"""
    problem, n, alpha, zmin = BATCHES[name][:4]
    opts = dict(alpha=alpha, zMin=zmin)
    return (problem, n, CAR, opts) if problem == "carparking" else (problem, n, BRACHI, dict(BRACHI_OPTS, **opts))


def inputs(name, gains, rnd):
    """(x0, u0, l, L) of one case; rnd varies the start without touching what decides the failures"""
    problem, n = BATCHES[name][:2]
    if problem == "carparking":
        x0 = np.array(CAR_X0) + rnd * np.array([2.0 ** -7, -2.0 ** -8, 2.0 ** -9, 0.0])
        l, L = np.zeros((n, 2)), np.zeros((n, 8))
        if gains[0] == "one":
            l[gains[1], 0] = gains[2]
        else:
            l[0, 0], l[1, 0], L[1, 0 + 2 * 2] = gains[1], -gains[2], gains[3]  # L is nu x nx, column-major: (w, t)
        return x0, np.zeros((n, 2)), l, L
    x0 = np.array([-0.5 - 0.03125 * rnd])
    l, L = np.zeros((n, 1)), np.zeros((n, 1))
    l[gains[1], 0] = gains[2]
    return x0, -np.ones((n, 1)), l, L


def margins(name, x, u):
    """per step of a candidate trajectory, how far the argument of the square root that can fail is from failing, relative:
    > 0 finite, < 0 failing.  CarParking: 1 - |h v sin w| / d; brachi: (-y - dy dx) / (|y| + |dy dx|)"""
    n = BATCHES[name][1]
    if BATCHES[name][0] == "carparking":
        return 1.0 - np.abs(CAR["h"][0] * x[:n, 3] * np.sin(u[:, 0])) / CAR["d"][0]
    dx = BRACHI["dx"][0]
    return (-x[:n, 0] - u[:, 0] * dx) / (np.abs(x[:n, 0]) + np.abs(u[:, 0] * dx))


def scalars_of(scal, ok, c, alpha):
    """(cost, dV0, dV1) of a scalars rule from the roll-outs' (ok, cost) per step size"""
    fin = [i for i in range(len(alpha)) if ok[i]]
    low, high = min([c[i] for i in fin] or [1.0]), max([c[i] for i in fin] or [1.0])
    if scal[0] == "first":
        j = scal[1]
        before = [c[i] for i in fin if i < j]
        if not ok[j]:  # (the all-fail cases: any cost)
            return 1.0, -1.0, 0.0
        hi = min(before) if before else c[j] + 2.0
        assert c[j] < hi, (scal, c)
        return 0.5 * (c[j] + hi), -1.0, 0.0
    if scal[0] == "none":
        return low - 1.0, -1.0, 0.0
    if scal[0] == "neg":
        t = scal[1]
        return low - 1.0, 1.0, -1.0 / np.sqrt(alpha[t] * alpha[t + 1])
    if scal[0] == "zero":
        return high + 1.0, 0.0, 0.0
    if scal[0] == "z":
        return c[scal[1]] + scal[2] * alpha[scal[1]], -1.0, 0.0
    if scal[0] == "tie":
        j = scal[1]
        cost = c[j] + 0.5 * alpha[j]
        for cand in _neighbours(cost, 16):
            if (cand - c[j]) / alpha[j] == 0.5:
                return cand, -1.0, 0.0
        raise AssertionError("no cost within 16 last places gives z == 0.5 exactly")
    raise ValueError(scal)


def _neighbours(v, n):
    out, up, down = [v], v, v
    for _ in range(n):
        up, down = np.nextafter(up, np.inf), np.nextafter(down, -np.inf)
        out += [up, down]
    return out


_built = {}
INT_FIELDS = ("ok", "idx", "ret", "cmp_new_cost", "cmp_dexp", "tie")
FIELDS = ("x0", "u0", "l", "L", "cost", "dV0", "dV1", "ac", "margin", "new_cost", "dcost", "expected", "xn", "un", "xc", "uc") + INT_FIELDS


def reference(name, kind="oracle"):
    """everything about batch `name` from the driver build `kind`, computed once per process: dict of arrays over the
    batch's trajectories —
      x0 u0 l L cost dV0 dV1      the inputs
      ok [B, A], ac [B, A]        Driver.forward_pass(alpha[i]) of every step size: succeeded, cost (NaN where it failed: the
                                  reference's partial sum is not the device's number)
      margin [B, A]               the smallest margins() over the steps of a finite roll-out, that of the failing step of a
                                  failed one (< 0), and the smallest of the steps in front of it in margin_front
      idx ret new_cost dcost expected   line_search(): log_linesearch, return value and what it leaves behind
      cmp_new_cost, cmp_dexp      whether new_cost / dcost and expected are compared (module docstring); NaN where not
      tie                         the deliberate z == zMin case
      xn un                       the nominal trajectory;  xc uc  the candidate behind line_search() (the accepted roll-out)
    and cls, the classes' names"""
    key = (name, kind)
    if key in _built:
        return _built[key]
    problem, n, params, opts = setup(name)
    alpha = BATCHES[name][2]
    A = len(alpha)
    rows = {k: [] for k in FIELDS + ("margin_front",)}
    cls = []
    for c_name, gains, scal, rnd in specs(name):
        x0, u0, l, L = inputs(name, gains, rnd)
        d = Driver(lib_path(kind, problem, 0), n, params, opts)
        assert d.init(x0, u0) == 1
        d.set_gains(l, L)
        ok, ac, mg, mf = np.zeros(A, dtype=np.int32), np.zeros(A), np.zeros(A), np.ones(A)
        for i, a in enumerate(alpha):
            ok[i], ac[i] = d.forward_pass(a)
            m = margins(name, *d.traj(1))
            if ok[i]:
                mg[i] = m.min()
            else:  # the candidate holds the steps up to the failing one: the first beyond the limit
                k = int(np.argmax(~(m > 0)))
                mg[i], mf[i] = m[k], (m[:k].min() if k else 1.0)
        cost, dV0, dV1 = scalars_of(scal, ok, ac, alpha)
        d.set_search_state(cost, dV0, dV1)
        ret = d.line_search(0)
        idx, sc = d.log_linesearch(0), d.scalars()
        tried = ok[:idx] if ret else ok
        cmp_new_cost, cmp_dexp = bool(tried[-1]), bool(tried.any())
        xn, un = d.traj(0)
        xc, uc = d.traj(1)
        d.close()
        vals = dict(x0=x0, u0=u0, l=l, L=L, cost=cost, dV0=dV0, dV1=dV1, ok=ok, ac=np.where(ok == 1, ac, np.nan), margin=mg, margin_front=mf,
                    idx=idx, ret=ret, new_cost=sc["new_cost"] if cmp_new_cost else np.nan, dcost=sc["dcost"] if cmp_dexp else np.nan,
                    expected=sc["expected"] if cmp_dexp else np.nan, cmp_new_cost=cmp_new_cost, cmp_dexp=cmp_dexp, tie=scal[0] == "tie",
                    xn=xn, un=un, xc=xc if ret else xn, uc=uc if ret else un)
        for k, v in vals.items():
            rows[k].append(v)
        cls.append(c_name)
    out = {k: np.array(v, dtype=np.int32 if k in INT_FIELDS else np.float64) for k, v in rows.items()}
    out["cls"] = cls
    _built[key] = out
    return out


def golden_of(kind="ref"):
    """what tests/golden/linesearch.npz records (tests/golden/make_goldens.py linesearch): the results of the reference
    build on every case — its roll-outs per step size, its line_search() and the trajectory it leaves"""
    out = {}
    for name in BATCHES:
        r = reference(name, kind)
        for k in ("cost", "dV0", "dV1", "ok", "ac", "idx", "ret", "new_cost", "dcost", "expected", "xc", "uc"):
            out[name + "/" + k] = r[k]
    return out


# ---------------------------------------------------------------------------
# sequences of searches: where the current trajectory lives (ls_keep = 2)
# ---------------------------------------------------------------------------
# Five iterations in a row on the demo's CarParking (every roll-out finite), the real stages calc_derivs, back_pass,
# line_search, update with lambda held at one value; only scalars steer the outcome, so that no host write of a trajectory
# brings the trajectories home between the searches.  Per trajectory and search the plan names what happens:
#   first     accepted in the first stage: the trajectory moves into a plane of the search's set
#   second    accepted in the second stage: copied into X / U (k_adopt_home)
#   reject    nothing accepted: a trajectory living in a plane is copied into X / U (k_adopt_home's else branch, or
#             k_rejected_home behind a search without a second stage)
# (a) all first; (b) a third each reject / second / first; (c) first / reject / second; (d) second / first / reject — the
# trajectories in a second stage of (c) and (d) and those rejected in (b) and (d) live in a plane then; (e) first and reject
# in turn, with another ls_split: plane_n changes, all_home runs.
# Index j is accepted exactly when the cost lies between the threshold f[j] = c[j] + zMin expected[j] and the lowest
# threshold in front of it, so j can be planned where f[j] is a record low of the list (by SEQ_GAP).
#   steer = "dV"    dV = (-SEQ_K, 0) set behind the backward pass: expected = SEQ_K alpha, f falls along the whole list
#                   (SEQ_K zMin (alpha[i] - alpha[i+1]) dwarfs the roll-outs' cost differences — asserted) and every index
#                   can be planned.  Staged calls only: iterate() leaves no place to set dV.
#   steer = "cost"  the backward pass's own dV, the cost alone steers: what iterate() allows.  With zMin = 0 the thresholds
#                   fall along the list only where the full step falls short of zMin times its promise.  Probed on the CPU:
#                   at n_hor 12 ... 40, or at lambda = 1, index 0 is the only record low of every search; at n_hor = 100,
#                   lambda = 0.03, zMin = 0.99 four to seven of the 16 trajectories a search plans `second` for have a
#                   record low behind index 1 — so the first stage takes two step sizes — while the reference's own
#                   sources built with FMA contraction stay within 4e-15 of the FMA-free build over the five iterations
#                   (at lambda <= 0.01 or n_hor >= 150 single trajectories leave by 1e-2 and more: no bar could hold).
#                   Where the planned stage has no record low, index 0 is taken.
SEQ_B, SEQ_K, SEQ_GAP = 48, 100.0, 1e-4
SEQ = {"dV": dict(n_hor=12, lam=1.0, zMin=0.5, splits=(4, 4, 4, 4, 3)), "cost": dict(n_hor=100, lam=0.03, zMin=0.99, splits=(2, 2, 2, 2, 1))}
SEQ_PLAN = (("first",) * 3, ("reject", "second", "first"), ("first", "reject", "second"), ("second", "first", "reject"), ("first", "reject", "first"))

_sequences = {}


def _thresholds(d, alpha, zmin, dV):
    """f[i] = c[i] + zMin expected[i] of the driver's nominal and gains: z[i] > zMin exactly when cost > f[i]"""
    rolls = [d.forward_pass(a) for a in alpha]
    expected = np.array([-a * (dV[0] + a * dV[1]) for a in alpha])
    assert all(r[0] == 1 for r in rolls) and np.all(expected > 0)
    return np.array([r[1] for r in rolls]) + zmin * expected


def _choose(want, f, s1, turn):
    """(index to accept or None, the cost that does exactly that): among the record lows of f in the wanted stage the one
    whose turn it is, index 0 where the stage has none"""
    if want == "reject":
        return None, f.min() - 1.0
    lows = [j for j in range(len(f)) if j == 0 or f[j] < f[:j].min() - SEQ_GAP]
    stage = [j for j in lows if (j < s1) == (want == "first")]
    j = stage[turn % len(stage)] if stage else 0
    return j, (0.5 * (f[j] + f[:j].min()) if j else f[0] + 1.0)


def sequence_reference(n_alpha, steer, kind="oracle"):
    """dict(steer, alpha, zMin, lam, n_hor, splits, x0, u0, cost [5, B], dV [5, B, 2], idx [5, B], ret [5, B], what [5][B] (first /
    second / reject as it happened), x [5, B, N + 1, 4], u [5, B, N, 2]: the nominal after each search) from the driver build `kind`"""
    key = (n_alpha, steer, kind)
    if key in _sequences:
        return _sequences[key]
    n, lam, zmin, splits = (SEQ[steer][k] for k in ("n_hor", "lam", "zMin", "splits"))
    alpha = ALPHA8[:n_alpha]
    rng = np.random.default_rng(20261020)
    x0 = np.array([1.0, 1.0, 1.5 * np.pi, 0.0]) + np.array([0.5, 0.5, 0.5, 0.2]) * rng.uniform(-1, 1, (SEQ_B, 4))
    u0 = 0.1 * rng.standard_normal((SEQ_B, n, 2))
    S = len(SEQ_PLAN)
    out = dict(steer=steer, alpha=alpha, zMin=zmin, lam=lam, n_hor=n, splits=splits, x0=x0, u0=u0, cost=np.zeros((S, SEQ_B)), dV=np.zeros((S, SEQ_B, 2)),
               idx=np.zeros((S, SEQ_B), dtype=np.int32), ret=np.zeros((S, SEQ_B), dtype=np.int32), what=[[None] * SEQ_B for _ in range(S)],
               x=np.zeros((S, SEQ_B, n + 1, 4)), u=np.zeros((S, SEQ_B, n, 2)))
    for b in range(SEQ_B):
        d = Driver(lib_path(kind, "carparking", 0), n, CAR_PARAMS, dict(alpha=alpha, zMin=zmin))
        assert d.init(x0[b], u0[b]) == 1
        for s in range(S):
            s1 = min(splits[s], n_alpha)
            d.set_lambda(lam)
            assert d.calc_derivs() == 1 and d.back_pass() == 0
            sc = d.scalars()
            dV = (-SEQ_K, 0.0) if steer == "dV" else (sc["dV0"], sc["dV1"])
            f = _thresholds(d, alpha, zmin, dV)
            if steer == "dV":
                assert np.all(np.diff(f) < -SEQ_GAP), (b, s, f)
            j, cost = _choose(SEQ_PLAN[s][b % 3], f, s1, b // 3)
            d.set_search_state(cost, *dV)
            ret = d.line_search(s)
            assert (ret, d.log_linesearch(s)) == ((1, j + 1) if j is not None else (0, n_alpha + 1)), (b, s, j, d.log_linesearch(s))
            if ret:
                d.accept()
            out["cost"][s, b], out["dV"][s, b], out["idx"][s, b], out["ret"][s, b] = cost, dV, d.log_linesearch(s), ret
            out["what"][s][b] = "reject" if j is None else ("first" if j < s1 else "second")
            out["x"][s, b], out["u"][s, b] = d.traj(0)
        d.close()
    _sequences[key] = out
    return out
