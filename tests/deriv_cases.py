"""The truth the derivative records are held to, from the problem's DEFINITION alone (no GPU).

Every parity test feeds both sides the same generated problem file, so a derivative tools/gen_problem.py gets wrong is wrong
alike in the oracle, in the reference build and in every kernel.  This module shares nothing with the generator but
`load_problem` and the fields of its `Problem` (x, u, params, aux, f, L, F, h, hle, hli, hfe, hfi): no Deriver, no Emitter, no
printer, no sympy.diff.  The auxiliaries are substituted into the definitions, the definitions are lambdified to mpmath, and
every derivative is a central difference in DPS-digit arithmetic with step H:

    g_i   = (g(z + H e_i) - g(z - H e_i)) / 2H                                     truncation ~ H^2 g''' / 6
    g_ii  = (g(z + H e_i) - 2 g(z) + g(z - H e_i)) / H^2                           truncation ~ H^2 g'''' / 12
    g_ij  = (g(++) - g(+-) - g(-+) + g(--)) / 4H^2                                 rounding   ~ 10^-DPS / H^2

With DPS = 80 and H = 1e-25 both are around 1e-30 of g's scale.  MEASURED (tests/test_deriv_cases_recipe.py, against the
closed-form derivatives of a hand-written function of sin, exp, a cube and a quotient): 2.2e-31 worst, first and second
derivatives alike — DIFF_ERROR below is the bound every user of this module may rely on.  A difference below SNAP times the
function's scale is a derivative that is identically zero (the structural zeros come out as 0 exactly where g does not depend
on z_i at all, and as rounding of size 1e-30 where it is linear in it); no non-zero derivative of these problems at these
points is below 1e-9.

THE AUGMENTATION, restated from the generator's docstring (genenerator_main.mac:46-124): a constraint h with multiplier mu
and penalty weight w adds to the cost
    equality                mu h + w h^2 / 2
    inequality, h >= 0      mu h (1 + w h)
    inequality, h <  0      mu h / (1 - w h)
the running constraints (hle, hli) to L with w = w_pen_l, the final ones (hfe, hfi) to F with w = w_pen_f.  (The generator's
code, that docstring and the reference's own text — genenerator_main.mac:54, 75, 94, 112 — state the same three forms.)

THE BOX AND ITS GRADIENTS (limitsU of the generated file; back_pass.c:186-199 reads them).  An input constraint is
h_i = s u_j + g(x) <= 0 with s = +-1.  s = +1 bounds u_j from above by u_j - h_i, s = -1 from below by u_j + h_i.  Per input
and side the TIGHTEST bound wins (the first of equal ones), and the record holds
    lower[j] / upper[j]            that bound MINUS u_j (the solver works with the change of u); -inf / +inf without one
    lower_sign[j] / upper_sign[j]  s of the winning constraint, 0 without one
    lower_hx / upper_hx [r + j n]  d h_i / d x_r of the winning constraint (of h itself, u_j's term included: not of the bound)
                                   zeros without one

THE RECORD, in the order of oracle/driver.c:drv_get_derivs:
    cx cxx cu cuu cxu fx fu lower upper [fxx fuu fxu] lower_sign upper_sign lower_hx upper_hx;   fin = cx cxx of augmented F
    fx[r + c n], fu[r + c n], cxu[r + c n];  packed upper triangles [c (c + 1) / 2 + r], r <= c;
    fxx[j + i sizeofQxx], fuu[j + i sizeofQuu] (j packed);  fxu[r + c n + i n m]   (i: the component of f)

THE POINTS: the states and inputs of a roll-out of N_HOR = 6 steps that the reference build's driver makes (the n = 16
problems: three steps of it), parameters from oracle/harness.py.  Multiplier problems: multipliers drawn non-zero, penalty
weights 2.0 (running) and 7.0 (final), and a start chosen so that every running inequality is met on both sides of zero
within the six steps with |h| > 1e-6 everywhere (the difference stencil stays inside one branch) — asserted by check_case().
A final inequality has one point per roll-out: AlMix has a second case (`almix_b`) for its other side.
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle.harness import (CAR_PARAMS, CAR_X0, HX_PARAMS, SYN10_PARAMS, SYN_PARAMS, SYNP_PARAMS, Driver, almix_case, brachi_case,  # noqa: E402
                            brachi_hli_case, lib_path, syn10_inputs, syn_inputs)

GOLDEN = os.path.join(ROOT, "tests", "golden", "deriv_truth.npz")
DPS, H_EXP = 80, -25
DIFF_ERROR = 1e-22   # bound on the differentiator's own error relative to the function's scale (measured: 2.2e-31)
SNAP = 1e-24
N_HOR = 6
W_PEN = (2.0, 7.0)
H_MARGIN = 1e-6


def tri(n):
    return n * (n + 1) // 2


def utri(r, c):
    return c * (c + 1) // 2 + r


# ---- the cases ------------------------------------------------------------------------------------------------------
def _almix(p0):
    params = dict(almix_case()[0])
    params["vref"] = np.asarray(params["vref"])[:N_HOR + 1]
    rng = np.random.default_rng(5)
    # gap = p - q = 16 pulls v down by about 0.4 a step: v from 0.9 through both velocity bounds (+-0.45) in six steps
    return params, np.array([p0, 0.9, p0 - 16.0]), 0.3 * rng.standard_normal((N_HOR, 2))


def _brachi(case):
    params = dict(case(N_HOR)[0])
    rng = np.random.default_rng(9)
    # (not the demos' y0 = -eps: sqrt(-y) has no derivatives there)
    return params, np.array([-0.3]), -1.0 + 0.2 * rng.uniform(-1, 1, (N_HOR, 1))


def _case(name):
    """(problem, FULL_DDP builds, params, x0, u0, steps whose records are held)"""
    every = tuple(range(N_HOR))
    if name == "carparking":
        rng = np.random.default_rng(7)
        return "carparking", (0, 1), CAR_PARAMS, np.array(CAR_X0) + 0.1, 0.3 * rng.standard_normal((N_HOR, 2)), every
    if name == "hxtest":
        rng = np.random.default_rng(20261003)
        return "hxtest", (0, 1), HX_PARAMS, np.array([-1.5, 0.0, 2.0]) + 0.3 * rng.standard_normal(3), 0.3 * rng.standard_normal((N_HOR, 2)), every
    if name in ("almix", "almix_b"):  # final position below (almix) and above (almix_b) its bound tgt[1] = 1.55
        params, x0, u0 = _almix(1.0 if name == "almix" else 2.0)
        return "almix", (0, 1), params, x0, u0, every
    if name == "brachi":
        params, x0, u0 = _brachi(brachi_case)
        return "brachi", (1,), params, x0, u0, every
    if name == "brachi_hli":
        params, x0, u0 = _brachi(brachi_hli_case)
        return "brachi_hli", (0, 1), params, x0, u0, every
    if name == "synth10hx":
        x0, u0 = syn10_inputs(1, N_HOR)
        return "synth10hx", (0, 1), SYN10_PARAMS, x0[0], u0[0], every
    if name == "synth16x8":
        x0, u0 = syn_inputs(1, N_HOR)
        return "synth16x8", (0, 1), SYN_PARAMS, x0[0], u0[0], (0, 3, 5)
    if name == "synth16p":
        x0, u0 = syn_inputs(1, N_HOR)
        return "synth16p", (1,), SYNP_PARAMS, x0[0], u0[0], (0, 3, 5)
    raise ValueError(name)


CASES = ("carparking", "hxtest", "almix", "almix_b", "brachi", "brachi_hli", "synth10hx", "synth16x8", "synth16p")
# the 14 problem builds (AlMix's second case runs on the same two)
BUILDS = [(name, fd) for name in CASES for fd in _case(name)[1]]


# ---- the definition as callables ------------------------------------------------------------------------------------
class Definition:
    """a problems/defs/*.py as mpmath callables of z = (x, u) at a step k; nothing but the Problem's fields is read"""

    def __init__(self, problem):
        import sympy as sp
        from tools.gen_problem import load_problem
        P = load_problem(os.path.join(ROOT, "problems", "defs", problem + ".py"))
        self.n, self.m = len(P.x), len(P.u)
        self.sizes = dict(P.params)
        aux = list(P.aux)

        def flat(e):
            e = sp.sympify(e)
            for s, d in reversed(aux):  # (an auxiliary may be defined through earlier ones)
                e = e.subs(s, d)
            return e

        self.exprs = dict(f=[flat(e) for e in P.f], L=[flat(P.L)], F=[flat(P.F)], h=[flat(e) for e in P.h],
                          hle=[flat(e) for e in P.hle], hli=[flat(e) for e in P.hli], hfe=[flat(e) for e in P.hfe], hfi=[flat(e) for e in P.hfi])
        self.z = list(P.x) + list(P.u)
        self.psyms = sorted(set().union(*[e.free_symbols for v in self.exprs.values() for e in v]) - set(self.z), key=lambda s: s.name)
        assert not any(set(P.u) & e.free_symbols for k in ("F", "hfe", "hfi") for e in self.exprs[k])
        self.fn = {k: sp.lambdify(self.z + self.psyms, v, "mpmath", cse=True) for k, v in self.exprs.items()}
        # (for the chain-rule mutant alone: f with the auxiliaries left in as further variables, and the auxiliaries)
        self.aux = aux
        self.raw = P

    def dims(self):
        """(running multipliers, final multipliers): mu_le then mu_li, mu_fe then mu_fi — the structs' member order"""
        e = self.exprs
        return len(e["hle"]) + len(e["hli"]), len(e["hfe"]) + len(e["hfi"])

    def pvals(self, params, k, shift=0):
        """the parameter symbols' values at step k (`name[k]`: entry k + shift of a per-step parameter)"""
        import mpmath as mp
        out = []
        for s in self.psyms:
            nm = s.name
            if nm.endswith("[k]"):
                out.append(mp.mpf(float(np.asarray(params[nm[:-3]])[k + shift])))
            elif "[" in nm:
                out.append(mp.mpf(float(params[nm[:nm.index("[")]][int(nm[nm.index("[") + 1:-1])])))
            else:
                out.append(mp.mpf(float(np.atleast_1d(params[nm])[0])))
        return out


def penalty(kind, mu, h, w, mutant=None):
    """the augmentation of one constraint (module docstring); kind 'e' or 'i'"""
    if kind == "e":
        return mu * h + w * h * h / 2
    upper = h >= 0
    if mutant == "branches_exchanged":
        upper = not upper
    return mu * h * (1 + w * h) if upper else mu * h / (1 - w * h)


class Point:
    """the callables of one step: f(z), the augmented L(z) or F(z), the input constraints h(z)"""

    def __init__(self, D, params, k, mul, w_pen, final=False, mutant=None):
        import mpmath as mp
        self.D, self.final, self.mutant = D, final, mutant
        self.p = D.pvals(params, k, 1 if (mutant == "vref_next" and not final) else 0)
        self.mu = [mp.mpf(float(v)) for v in mul]
        w = w_pen[1] if (final or mutant == "w_pen_f_running") else w_pen[0]
        self.w = mp.mpf(float(w))

    def _call(self, key, z):
        pad = [0] * self.D.m if self.final else []  # (F and the final constraints do not depend on u)
        return self.D.fn[key](*(list(z) + pad + self.p))

    def f(self, z):
        return self._call("f", z)

    def h(self, z):
        return self._call("h", z)

    def cost(self, z):
        e, i = ("hfe", "hfi") if self.final else ("hle", "hli")
        c = self._call("F" if self.final else "L", z)[0]
        he, hi = self._call(e, z), self._call(i, z)
        for j, h in enumerate(he):
            c = c + penalty("e", self.mu[j], h, self.w)
        for j, h in enumerate(hi):
            c = c + penalty("i", self.mu[len(he) + j], h, self.w, self.mutant)
        return [c]

    def inequalities(self, z):
        return self._call("hfi" if self.final else "hli", z)


# ---- the differentiator ---------------------------------------------------------------------------------------------
def _snap(v, scale):
    return [a if abs(a) > SNAP * scale else 0 * a for a in v]


def jacobian(g, z):
    """J[i][q] = d g_q / d z_i by central differences (module docstring)"""
    import mpmath as mp
    h = mp.mpf(10) ** H_EXP
    J = []
    for i in range(len(z)):
        zp, zm = list(z), list(z)
        zp[i] = z[i] + h
        zm[i] = z[i] - h
        gp, gm = g(zp), g(zm)
        J.append([(a - b) / (2 * h) for a, b in zip(gp, gm)])
    scale = max([1] + [abs(a) for a in g(z)])
    return [_snap(row, scale) for row in J]


def hessian(g, z):
    """Hs[i][j][q] = d^2 g_q / d z_i d z_j, i <= j, by central differences; Hs[j][i] is the same list"""
    import mpmath as mp
    h = mp.mpf(10) ** H_EXP
    d = len(z)
    g0 = g(z)
    scale = max([1] + [abs(a) for a in g0])
    Hs = [[None] * d for _ in range(d)]

    def at(i, si, j=None, sj=0):
        w = list(z)
        w[i] = w[i] + si * h
        if j is not None:
            w[j] = w[j] + sj * h
        return g(w)

    for i in range(d):
        gp, gm = at(i, 1), at(i, -1)
        Hs[i][i] = _snap([(a - 2 * c + b) / (h * h) for a, b, c in zip(gp, gm, g0)], scale)
        for j in range(i + 1, d):
            pp, pm, mp_, mm = at(i, 1, j, 1), at(i, 1, j, -1), at(i, -1, j, 1), at(i, -1, j, -1)
            Hs[i][j] = Hs[j][i] = _snap([(a - b - c + e) / (4 * h * h) for a, b, c, e in zip(pp, pm, mp_, mm)], scale)
    return Hs


# ---- the record of one step -----------------------------------------------------------------------------------------
def segments(n, m, fd, final=False):
    """[(array, length)] of a record in drv_get_derivs's order"""
    if final:
        return [("cx", n), ("cxx", tri(n))]
    s = [("cx", n), ("cxx", tri(n)), ("cu", m), ("cuu", tri(m)), ("cxu", n * m), ("fx", n * n), ("fu", n * m), ("lower", m), ("upper", m)]
    if fd:
        s += [("fxx", n * tri(n)), ("fuu", n * tri(m)), ("fxu", n * n * m)]
    return s + [("lower_sign", m), ("upper_sign", m), ("lower_hx", n * m), ("upper_hx", n * m)]


def split(rec, n, m, fd, final=False):
    out, o = {}, 0
    for name, cnt in segments(n, m, fd, final):
        out[name] = rec[..., o:o + cnt]
        o += cnt
    assert o == rec.shape[-1], (o, rec.shape)
    return out


def join(parts, n, m, fd, final=False):
    return np.concatenate([parts[name] for name, _ in segments(n, m, fd, final)], axis=-1)


def drop_tensors(rec, n, m):
    """the FULL_DDP = 0 record out of the FULL_DDP = 1 one"""
    return join(split(rec, n, m, 1), n, m, 0)


def box(pt, z, n, m):
    """lower, upper, lower_sign, upper_sign, lower_hx, upper_hx by the rule of the module docstring"""
    import mpmath as mp
    hv = pt.h(z)
    J = jacobian(pt.h, z) if hv else []
    bound = [[-mp.inf] * m, [mp.inf] * m]
    sign = [[0.0] * m, [0.0] * m]
    grad = [[0.0] * (n * m), [0.0] * (n * m)]
    for i, h in enumerate(hv):
        hu = [J[n + j][i] for j in range(m)]
        nz = [j for j in range(m) if hu[j] != 0]
        assert len(nz) == 1 and abs(abs(hu[nz[0]]) - 1) < DIFF_ERROR, "an input constraint is s u_j + g(x) with s = +-1"
        j, s = nz[0], (1 if hu[nz[0]] > 0 else -1)
        side = 1 if s > 0 else 0
        b = z[n + j] - h if s > 0 else z[n + j] + h
        if (b < bound[1][j]) if side else (b > bound[0][j]):
            bound[side][j] = b
            sign[side][j] = float(s)
            for r in range(n):
                grad[side][r + j * n] = float(J[r][i])
    lower = [float(bound[0][j] - z[n + j]) for j in range(m)]
    upper = [float(bound[1][j] - z[n + j]) for j in range(m)]
    return lower, upper, sign[0], sign[1], grad[0], grad[1]


def truth_step(pt, x, u, n, m):
    """the FULL_DDP = 1 record of one running step"""
    import mpmath as mp
    z = [mp.mpf(float(v)) for v in x] + [mp.mpf(float(v)) for v in u]
    Jc, Hc = jacobian(pt.cost, z), hessian(pt.cost, z)
    Jf, Hf = jacobian(pt.f, z), hessian(pt.f, z)
    X, U = range(n), range(n, n + m)
    lower, upper, ls, us, lhx, uhx = box(pt, z, n, m)
    p = dict(
        cx=[Jc[r][0] for r in X],
        cxx=[Hc[r][c][0] for c in X for r in range(c + 1)],
        cu=[Jc[r][0] for r in U],
        cuu=[Hc[n + r][n + c][0] for c in range(m) for r in range(c + 1)],
        cxu=[Hc[r][n + c][0] for c in range(m) for r in X],
        fx=[Jf[c][r] for c in X for r in X],
        fu=[Jf[n + c][r] for c in range(m) for r in X],
        lower=lower, upper=upper,
        fxx=[Hf[r][c][i] for i in X for c in X for r in range(c + 1)],
        fuu=[Hf[n + r][n + c][i] for i in X for c in range(m) for r in range(c + 1)],
        fxu=[Hf[r][n + c][i] for i in X for c in range(m) for r in X],
        lower_sign=ls, upper_sign=us, lower_hx=lhx, upper_hx=uhx)
    return join({k: np.array([float(v) for v in a], dtype=np.float64) for k, a in p.items()}, n, m, 1)


def truth_final(pt, x, n):
    import mpmath as mp
    z = [mp.mpf(float(v)) for v in x]
    J, Hs = jacobian(pt.cost, z), hessian(pt.cost, z)
    return np.array([float(J[r][0]) for r in range(n)] + [float(Hs[r][c][0]) for c in range(n) for r in range(c + 1)])


def values(D, params, xs, us, el, fin, w_pen):
    """f(x_k, u_k), the augmented L at every step and the augmented F, correctly rounded: what forward_pass is held to"""
    import mpmath as mp
    mp.mp.dps = DPS
    N = len(us)
    nxt, cost = np.zeros((N, D.n)), np.zeros(N + 1)
    for k in range(N):
        pt = Point(D, params, k, el[k], w_pen)
        z = [mp.mpf(float(v)) for v in xs[k]] + [mp.mpf(float(v)) for v in us[k]]
        nxt[k] = [float(v) for v in pt.f(z)]
        cost[k] = float(pt.cost(z)[0])
    cost[N] = float(Point(D, params, N, fin, w_pen, final=True).cost([mp.mpf(float(v)) for v in xs[N]])[0])
    return nxt, cost


def truth(D, params, xs, us, el, fin, w_pen, steps, mutant=None):
    """(rec [len(steps), FULL_DDP = 1 record], fin record) at the points of the roll-out (xs, us)"""
    import mpmath as mp
    mp.mp.dps = DPS
    rec = np.array([truth_step(Point(D, params, k, el[k], w_pen, mutant=mutant), xs[k], us[k], D.n, D.m) for k in steps])
    return rec, truth_final(Point(D, params, len(us), fin, w_pen, final=True, mutant=mutant), xs[len(us)], D.n)


# ---- the roll-out, the multipliers, the records of a build ----------------------------------------------------------
_defs = {}


def definition(problem):
    if problem not in _defs:
        _defs[problem] = Definition(problem)
    return _defs[problem]


def multipliers_of(name):
    """(running [N_HOR, el], final [fin]) drawn non-zero (0.5 .. 1.5), the same for every build of the case"""
    D = definition(_case(name)[0])
    ne, nf = D.dims()
    rng = np.random.default_rng(31)
    return rng.uniform(0.5, 1.5, (N_HOR, ne)), rng.uniform(0.5, 1.5, nf)


def struct_members(D, el, fin):
    """the multiplier structs member by member (iLQG_problem.tem:70-89): per kind the multipliers, then as many `last_h`
    (what update_multipliers remembers: no derivative reads them; zeros)"""
    def members(mu, counts):
        mu = np.atleast_2d(mu)
        cols, o = [], 0
        for c in counts:
            cols += [mu[:, o:o + c], np.zeros((len(mu), c))]
            o += c
        return np.concatenate(cols, axis=1) if cols else np.zeros((len(mu), 0))
    e = D.exprs
    return members(el, (len(e["hle"]), len(e["hli"]))), members(fin, (len(e["hfe"]), len(e["hfi"])))[0]


def swept_driver(name, fd, kind, point=None):
    """(driver, xs, us) up to and with the cost re-sweep of records()'s sequence; the caller closes it"""
    problem, _, params, x0, u0, _ = _case(name)
    el, fin = multipliers_of(name)
    d = Driver(lib_path(kind, problem, fd), N_HOR, params, dict(max_iter=1))
    assert d.init(x0, u0) == 1
    xs, us = d.traj(0) if point is None else point
    if el.shape[1] or len(fin):
        d.set_multipliers(*struct_members(definition(problem), el, fin))
    d.set_state(xs, us, 0.0, 1.0, W_PEN)
    assert d.cost_resweep() == 1
    return d, xs, us


def records(name, fd, kind, point=None):
    """The records of a driver build at the case's points, by the sequence the driver needs: init (its own roll-out),
    set_multipliers, set_state with the roll-out's own x, u and the penalty weights, cost_resweep (forward_pass over the
    nominal again: the auxiliaries stored in the trajectory then belong to THESE multipliers and weights — a record behind
    set_state alone would use the ones init left), calc_derivs.  point = (xs, us): these states and inputs in place of the
    build's own roll-out.  -> dict(xs, us, rec [steps], fin, step_costs)"""
    steps = _case(name)[5]
    d, xs, us = swept_driver(name, fd, kind, point)
    assert d.calc_derivs() == 1
    rec, rfin = d.derivs()
    out = dict(xs=xs, us=us, rec=rec[list(steps)], fin=rfin, step_costs=d.step_costs(0))
    d.close()
    return out


_truths = {}


def case_truth(name):
    """dict(params.., xs, us, el, fin_mul, w_pen, steps, rec, fin, next, cost) of a case: the points are the reference
    build's roll-out where that build exists, else the oracle's (the golden file has the reference's)"""
    if name in _truths:
        return _truths[name]
    problem, fds, params, x0, u0, steps = _case(name)
    D = definition(problem)
    kind = "ref" if os.path.exists(lib_path("ref", problem, fds[-1])) else "oracle"
    r = records(name, fds[-1], kind)
    el, fin = multipliers_of(name)
    rec, rfin = truth(D, params, r["xs"], r["us"], el, fin, W_PEN, steps)
    nxt, cost = values(D, params, r["xs"], r["us"], el, fin, W_PEN)
    _truths[name] = dict(xs=r["xs"], us=r["us"], el=el, fin_mul=fin, w_pen=np.array(W_PEN), steps=np.array(steps, dtype=np.float64),
                         rec=rec, fin=rfin, next=nxt, cost=cost)
    return _truths[name]


def check_case(name):
    """what the case was chosen for: every running inequality on both sides of zero within the roll-out, the final one of
    AlMix on one side per case, |h| > H_MARGIN everywhere"""
    import mpmath as mp
    mp.mp.dps = DPS
    problem, _, params, _, _, _ = _case(name)
    D, t = definition(problem), case_truth(name)
    seen = []
    for k in range(N_HOR):
        pt = Point(D, params, k, t["el"][k], W_PEN)
        seen.append([float(v) for v in pt.inequalities([mp.mpf(float(v)) for v in list(t["xs"][k]) + list(t["us"][k])])])
    seen = np.array(seen)
    final = np.array([float(v) for v in Point(D, params, N_HOR, t["fin_mul"], W_PEN, final=True).inequalities([mp.mpf(float(v)) for v in t["xs"][N_HOR]])])
    assert np.all(np.abs(seen) > H_MARGIN) and np.all(np.abs(final) > H_MARGIN), (name, seen, final)
    if seen.shape[1]:
        assert np.all(seen.max(axis=0) > 0) and np.all(seen.min(axis=0) < 0), (name, seen)
    return seen, final


# ---- the measure ----------------------------------------------------------------------------------------------------
def error(got, want, n, m, fd, final=False, only=None):
    """The worst entry of |got - want| / max |want over its array at its step| (per array of the record, per step: an entry
    of size 1e-6 in an array of that size is held as tightly as one of size 1).  An array that is identically zero in
    `want`, and every entry that is not finite there, must be EQUAL in `got`: inf is returned otherwise.  only: these arrays."""
    got, want = np.atleast_2d(got), np.atleast_2d(want)
    worst = 0.0
    g, w = split(got, n, m, fd, final), split(want, n, m, fd, final)
    for name in (only or w):
        for a, b in zip(g[name], w[name]):
            fin = np.isfinite(b)
            if not np.array_equal(a[~fin], b[~fin]):
                return np.inf
            scale = np.abs(b[fin]).max() if fin.any() else 0.0
            if scale == 0.0:
                if np.any(a[fin] != 0.0):
                    return np.inf
                continue
            worst = max(worst, float(np.abs(a[fin] - b[fin]).max() / scale))
    return worst


def build_error(name, fd, kind, t=None):
    """the worst normalised error of a build's records of a case, running and final"""
    problem = _case(name)[0]
    D = definition(problem)
    t = t or case_truth(name)
    r = records(name, fd, kind, (t["xs"], t["us"]))
    want = t["rec"] if fd else drop_tensors(t["rec"], D.n, D.m)
    return max(error(r["rec"], want, D.n, D.m, fd), error(r["fin"], t["fin"], D.n, D.m, fd, final=True))


def key_of(name, fd):
    return "%s/fd%d/ref_error" % (name, fd)


def tensor_tables(problem, kind):
    """(coef, slice) of the problem's factored tensors out of a '*_forms' build, None where the generated file has none"""
    path = lib_path(kind + "_forms", problem, 1)
    d = Driver(path, N_HOR)
    out = d.tensor_tables() if "factored_tensors" in d.forms() else None
    d.close()
    return out


def truth_products(rec1, n, m, coef, sl):
    """The factored tensors' shared products AT THE TRUTH: every entry of slice i of fxx / fuu / fxu is a table number times
    product slice[i], so the product is the truth's entry over the table's number (taken where that number is largest).
    What the number IS is held by test_deriv_forms.py (coef * basis against the truth's whole tensors).  [steps, NBASIS]"""
    s = split(rec1, n, m, 1)
    out = np.zeros((len(rec1), int(sl.max()) + 1))
    off = 0
    for q, (nm, per) in enumerate((("fxx", tri(n)), ("fuu", tri(m)), ("fxu", n * m))):
        ten, c = s[nm].reshape(len(rec1), n, per), coef[off:off + n * per].reshape(n, per)
        off += n * per
        for i in range(n):
            if np.any(c[i] != 0.0):
                e = int(np.argmax(np.abs(c[i])))
                out[:, sl[q, i]] = ten[:, i, e] / c[i, e]
    return out


# ---- mutants: each is one way a record can be wrong; applied to a copy of the truth, never to a generated file -------------
MUTANTS = ("fx_transposed", "packed_row_major", "fxu_swapped", "chain_term_dropped", "branches_exchanged", "w_pen_f_running",
           "off_diagonal_doubled", "lower_hx_sign", "vref_next")


def mutated(name, mutant):
    """(rec, fin) of the FULL_DDP = 1 truth of a case with one mistake in it, or None where the case has nothing the
    mistake could touch"""
    problem, _, params, _, _, steps = _case(name)
    D, t = definition(problem), case_truth(name)
    n, m = D.n, D.m
    s = {k: v.copy() for k, v in split(t["rec"], n, m, 1).items()}
    fin = t["fin"].copy()
    S = len(steps)
    if mutant == "fx_transposed":
        s["fx"] = s["fx"].reshape(S, n, n).transpose(0, 2, 1).reshape(S, -1)
    elif mutant == "packed_row_major":  # entry (r, c), r <= c, at its place in a row-major upper triangle
        order = [utri(r, c) for r in range(n) for c in range(r, n)]
        s["cxx"] = s["cxx"][:, order]
        fin[n:] = fin[n:][order]
    elif mutant == "fxu_swapped":  # fxu[c + r m + i n m]
        s["fxu"] = s["fxu"].reshape(S, n, m, n).transpose(0, 1, 3, 2).reshape(S, -1)
    elif mutant == "off_diagonal_doubled":  # (the first off-diagonal entry of every packed Hessian of the dynamics and the cost)
        if n < 2:
            return None
        s["cxx"][:, utri(0, 1)] *= 2.0
        s["fxx"].reshape(S, n, tri(n))[:, :, utri(0, n - 1)] *= 2.0
    elif mutant == "lower_hx_sign":
        s["lower_hx"] = -s["lower_hx"]
    elif mutant == "chain_term_dropped":
        # f = g(z, a(z)):  f_rc = g_rc + g_ra a_c + g_ca a_r + g_aa a_r a_c + g_a a_rc.  The last term left out of ONE entry,
        # the first auxiliary's, in the first component of f that reads it, at the first pair (r, c) where a_rc is not 0
        import mpmath as mp
        import sympy as sp
        if len(D.aux) != 1:
            return None  # (one auxiliary, so that "f with the auxiliary left in" needs no further substitution)
        mp.mp.dps = DPS
        a_sym, a_def = D.aux[0]
        i = next(q for q, e in enumerate(D.raw.f) if a_sym in sp.sympify(e).free_symbols)
        g = sp.lambdify(D.z + [a_sym] + D.psyms, [D.raw.f[i]], "mpmath")
        a = sp.lambdify(D.z + D.psyms, [a_def], "mpmath")
        for j, k in enumerate(steps):
            p = D.pvals(params, k)
            z = [mp.mpf(float(v)) for v in list(t["xs"][k]) + list(t["us"][k])]
            a0 = a(*(z + p))[0]
            g_a = jacobian(lambda w: g(*(z + [w[0]] + p)), [a0])[0][0]
            A = hessian(lambda w: a(*(list(w) + p)), z)
            rc = next(((r, c) for c in range(n) for r in range(c + 1) if A[r][c][0] != 0), None)
            if rc is None:
                return None  # (an auxiliary that is linear in the state)
            r, c = rc
            s["fxx"][j, i * tri(n) + utri(r, c)] -= float(g_a * A[r][c][0])
    elif mutant in ("branches_exchanged", "w_pen_f_running", "vref_next"):
        if mutant == "vref_next" and not any(v == -1 for v in D.sizes.values()):
            return None
        if mutant == "w_pen_f_running" and not D.exprs["hle"] + D.exprs["hli"]:
            return None
        if mutant == "branches_exchanged" and not D.exprs["hli"] + D.exprs["hfi"]:
            return None
        return truth(D, params, t["xs"], t["us"], t["el"], t["fin_mul"], W_PEN, steps, mutant=mutant)
    else:
        raise ValueError(mutant)
    return join(s, n, m, 1), fin


def golden_of(kind="ref"):
    """tests/golden/deriv_truth.npz: per case the points, multipliers, weights, steps and the truth (float64), per build the
    measured worst normalised error of `kind`'s records; the parameters are the case's own (oracle/harness.py), stored too"""
    out = {}
    for name in CASES:
        problem, fds, params, _, _, _ = _case(name)
        t = case_truth(name)
        for k, v in t.items():
            out["%s/%s" % (name, k)] = np.asarray(v, dtype=np.float64)
        for pk, pv in params.items():
            out["%s/param/%s" % (name, pk)] = np.asarray(pv, dtype=np.float64)
        # (the multipliers as the structs hold them, for users without the definition: the GPU tests)
        out["%s/el_struct" % name], out["%s/fin_struct" % name] = struct_members(definition(problem), t["el"], t["fin_mul"])
        for fd in fds:
            out[key_of(name, fd)] = np.array(build_error(name, fd, kind))
        tables = tensor_tables(problem, kind)
        if tables is not None:
            D = definition(problem)
            out["%s/products" % name] = truth_products(t["rec"], D.n, D.m, *tables)
    return out
