"""TEST INFRASTRUCTURE — shared builders of the iteration-history tests (BatchSolver.set_history / history):
tests/test_history_binding.py and tests/test_history_recipe.py (no GPU) and tests/test_gpu_history.py.

An entry is what the per-trajectory fields hold at the return of line_search(), i.e. what oracle/driver.c records per line
search (Driver.trace(): lambda g_norm dV0 dV1 cost new_cost alpha_idx bp_calls) plus z, the iteration index and, with
multipliers, the penalty weights."""
import numpy as np

DOUBLES = ("cost", "new_cost", "z", "lambda", "g_norm", "dV0", "dV1")
PENALTIES = ("w_pen_l", "w_pen_f")  # libraries of problems with multipliers only
INTS = ("alpha_idx", "bp_calls", "iterations")
TRACE = ("lambda", "g_norm", "dV0", "dV1", "cost", "new_cost", "alpha_idx", "bp_calls")  # the fields of Driver.trace()
# the step sizes of standard_parameters() (ilqg_host.c; tests/test_history_binding.py holds the two lists together)
DEFAULT_ALPHA = (1.0, 0.3727594, 0.1389495, 0.0517947, 0.0193070, 0.0071969, 0.0026827, 0.0010000)


def z_recipe(cost, new_cost, alpha, dV0, dV1):
    """(dcost, expected, z) of an ACCEPTED step of size alpha, line_search.c:42-45, in its order of operations"""
    cost, new_cost, alpha, dV0, dV1 = (np.asarray(a, dtype=np.float64) for a in (cost, new_cost, alpha, dV0, dV1))
    dcost = cost - new_cost
    expected = -alpha * (dV0 + alpha * dV1)
    return dcost, expected, dcost / expected


def names_of(s):
    """every name history() of solver s returns"""
    return DOUBLES + (PENALTIES if sum(s.multiplier_dims()) else ()) + INTS + ("n",)


def valid(h, b):
    """trajectory b's entries that were written: {name: [min(n, cap)]}"""
    cap = h["alpha_idx"].shape[1]
    m = min(int(h["n"][b]), cap)
    return {k: v[b, :m] for k, v in h.items() if k != "n"}


def histories_equal(a, b, what, rows_a=slice(None), rows_b=slice(None)):
    """every field, every position (unwritten ones included: both read as zero), and the counts — bit for bit"""
    assert set(a) == set(b), what
    for k in a:
        x, y = np.asarray(a[k])[rows_a], np.asarray(b[k])[rows_b]
        assert x.shape == y.shape and np.array_equal(x, y), "%s: history field %s differs" % (what, k)


def unwritten_are_zero(h, what):
    cap = h["alpha_idx"].shape[1]
    beyond = np.arange(cap)[None, :] >= np.minimum(h["n"], cap)[:, None]
    for k, v in h.items():
        if k != "n":
            assert np.all(v[beyond] == 0), "%s: unwritten entries of %s are not zero" % (what, k)


def poll(s):
    """what an entry holds, read through the host between line_search() and update(): {name: [B]} and who is active"""
    out = {k: s.scalar(k).copy() for k in ("cost", "new_cost", "lambda", "g_norm", "dV0", "dV1")}
    dcost, expected = s.scalar("dcost"), s.scalar("expected")
    with np.errstate(all="ignore"):
        out["z"] = np.where(expected > 0, dcost / expected, 0.0)  # reduction_ratio of ilqg_rules.h
    if sum(s.multiplier_dims()):
        out.update({k: s.scalar(k).copy() for k in PENALTIES})
    out.update({k: s.ints(k).copy() for k in INTS})
    return out, s.ints("status") == 0


def staged(s, iterations, cap, stored):
    """`iterations` iterations stage by stage on solver s, the fields read between the search and the update: the history a
    recording batch must hold, {name: [B, cap]} and n.  stored: derivative records in HBM (calc_derivs + back_pass) as
    iterate() of a batch with fuse_derivs = 0 runs them; else the fused sweep."""
    B = s.B
    h = {k: np.zeros((B, cap), dtype=np.int32 if k in INTS else np.float64) for k in names_of(s) if k != "n"}
    n = np.zeros(B, dtype=np.int32)
    for _ in range(iterations):
        if stored:
            s.calc_derivs()
            s.back_pass()
        else:
            s.back_pass(fused=True)
        s.line_search()
        got, active = poll(s)
        for b in np.flatnonzero(active):
            if n[b] < cap:
                for k in h:
                    h[k][b, n[b]] = got[k][b]
            n[b] += 1
        s.update()
    h["n"] = n
    return h


def full_state(s):
    """every solver output a recording batch must share with one that does not record"""
    out = dict(x=s.x(), u=s.u())
    out["l"], out["L"] = s.gains()
    for k in ("cost", "new_cost", "dcost", "expected", "lambda", "dlambda", "g_norm", "dV0", "dV1", "alpha_cost"):
        out[k] = s.scalar(k)
    for k in ("status", "iterations", "alpha_idx", "accepted", "bp_calls", "need_derivs"):
        out[k] = s.ints(k)
    if sum(s.multiplier_dims()):
        out["mul"], out["mul_fin"] = s.multipliers()
        out["w_pen_l"], out["w_pen_f"] = s.scalar("w_pen_l"), s.scalar("w_pen_f")
    return out


def states_equal(a, b, what, rows_a=slice(None), rows_b=slice(None)):
    for k in a:
        assert np.array_equal(np.asarray(a[k])[rows_a], np.asarray(b[k])[rows_b], equal_nan=True), "%s: %s differs" % (what, k)


def launches(s):
    return {k: n for k, (n, _) in s.kernel_times().items()}
