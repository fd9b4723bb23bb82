"""BatchSolver.solve_stream(params=..., param_steps=..., history=...) on the GPU: a stream of starts that each bring a row
of fixed-size parameters, a window per per-time-step parameter and an iteration history of their own
(ilqg_batch_solve_stream_rows; finished starts come back through k_harvest).

A start of a stream is solved as a plain solve() solves it in a batch that holds it under set_params_batch /
set_param_steps_batch with its rows, bit for bit in every build: tests 1, 3, 4, 5, 6 and 7 are such identities (the plain
solves themselves are held to the CPU oracle stage by stage by tests/test_gpu_params_batch.py and
tests/test_gpu_param_steps.py).  Test 2 holds the FMA-free almix FULL_DDP 1 build — the one tests/test_gpu_history.py holds to
the reference's trace — to the CPU oracle's driver, start by start, bit for bit.  Inputs and shapes:
tests/stream_rows_cases.py (B = 70 slots, 230 starts); tests/test_solve_stream_rows_recipe.py pins, without a GPU, that these
starts finish at different iterations and that their rows change every cost."""
import ctypes as C
import os

import numpy as np
import pytest

from history_cases import DEFAULT_ALPHA, TRACE, histories_equal, launches, unwritten_are_zero, valid, z_recipe
from oracle.harness import lib_path
from stream_rows_cases import B, BUILDS, TOTAL, Inputs, oracle_solve
from test_gpu_receding_plant import assert_state_equal, full_state

pytestmark = pytest.mark.gpu

KEYS = ("cost", "status", "iterations", "x", "u")


@pytest.fixture(scope="module")
def ilqg():
    import __graft_entry__ as g
    g.load_package()
    from ddp_generator_amd import ilqg as m
    if not all(os.path.exists(m.library_path(*build)) for build in BUILDS.values()):
        g.build_for_tests()
    if m.Problem("carparking", 0).device_count() < 1:
        pytest.fail("no HIP device visible: the GPU tests must run on the MI355X box")
    return m


_inputs, _results = {}, {}


def inputs(name, total=TOTAL):
    if (name, total) not in _inputs:
        _inputs[name, total] = Inputs(name, total)
    return _inputs[name, total]


def has_rows(inp):
    """lane-mapped libraries carry parameters per trajectory; the wave mapping's are streamed without (history only)"""
    return inp.problem != "synth16x8" and inp.strict != "wave"


def make(ilqg, inp, batch, groups=0):
    kw = dict(groups=groups) if groups else {}
    return ilqg.BatchSolver(inp.problem, inp.fd, batch=batch, n_hor=inp.N, params=inp.params, opts=inp.opts, strict=inp.strict, **kw)


def run_stream(s, inp, sel=slice(None), rows=True, history=0, trajectories=True, table=None):
    rows = rows and has_rows(inp)
    table = inp.rows if table is None else table
    out = s.solve_stream(inp.x0[sel], inp.u0[sel], with_trajectories=trajectories,
                         params={n: t[sel] for n, t in table.items()} if rows else None,
                         param_steps={n: t[sel] for n, t in inp.steps.items()} if rows and inp.steps else None, history=history)
    out["trace"], out["counts"] = s.solve_trace(), s.stream_counts()
    return out


def streamed(ilqg, name, rows=True, history=0, trajectories=True, total=TOTAL, batch=B):
    """the stream of `name`, computed once and left unchanged"""
    key = ("stream", name, rows, history, trajectories, total, batch)
    if key not in _results:
        inp = inputs(name, total)
        s = make(ilqg, inp, batch)
        _results[key] = run_stream(s, inp, rows=rows, history=history, trajectories=trajectories)
        s.close()
    return _results[key]


def plain(ilqg, name, rows=True, history=0, total=TOTAL):
    """plain solves of the same starts in batches of at most 256 under set_params_batch / set_param_steps_batch with their
    rows, computed once and left unchanged: the KEYS, and `history` if a capacity is given"""
    key = ("plain", name, rows, history, total)
    if key in _results:
        return _results[key]
    inp = inputs(name, total)
    ref, hist = {k: [] for k in KEYS}, []
    for first in range(0, total, 256):
        sel = slice(first, min(total, first + 256))
        s = make(ilqg, inp, sel.stop - sel.start)
        if rows and has_rows(inp):
            s.set_params_batch({n: t[sel] for n, t in inp.rows.items()})
            for n, t in inp.steps.items():
                s.set_param_steps_batch(n, t[sel])
        if history:
            s.set_history(history)
        s.init(inp.x0[sel], inp.u0[sel])
        s.solve()
        got = dict(cost=s.scalar("cost"), status=s.ints("status"), iterations=s.ints("iterations"), x=s.x(), u=s.u())
        for k in KEYS:
            ref[k].append(np.array(got[k]))
        if history:
            hist.append(s.history())
        s.close()
    out = {k: np.concatenate(v) for k, v in ref.items()}
    if history:
        out["history"] = {k: np.concatenate([h[k] for h in hist]) for k in hist[0]}
    _results[key] = out
    return out


def results_equal(got, want, what, rows_got=slice(None), rows_want=slice(None), keys=KEYS):
    for k in keys:
        assert np.array_equal(np.asarray(got[k])[rows_got], np.asarray(want[k])[rows_want], equal_nan=True), "%s: %s differs" % (what, k)


# ---------------------------------------------------------------------------
# 1. a stream is its starts
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["carparking", "carparking_strict", "hxtest", "almix"])
def test_a_stream_with_rows_equals_plain_solves_under_the_same_rows(ilqg, name):
    """cost, status, iterations, x and u of every start, bit for bit; the stream refilled while others iterated, the starts
    finish at different iterations, all finish, and the rows are no no-op (more than half the costs differ from the same
    stream without rows)"""
    got, want = streamed(ilqg, name), plain(ilqg, name)
    results_equal(got, want, name)
    it, act, slots, refills = got["trace"]
    assert refills >= 4 and np.all(slots == B) and act.max() <= B, (refills, act)
    # the first poll finds nothing started and the last nothing left; at every poll between them — where the later refills
    # happen — trajectories are being iterated
    assert act[0] == 0 and act[-1] == 0 and np.all(act[1:-1] > 0), act
    assert len(np.unique(got["iterations"])) >= 4 and (got["status"] != 0).all()
    shared = streamed(ilqg, name, rows=False, trajectories=False)
    assert (shared["cost"] != got["cost"]).sum() > TOTAL // 2
    assert got["counts"]["contexts"] == 1


# ---------------------------------------------------------------------------
# 2. against the CPU oracle's driver, start by start
# ---------------------------------------------------------------------------
def test_every_start_is_its_own_oracle_solve_and_trace(ilqg, oracle_built):
    """FMA-free almix FULL_DDP 1, rows of tgt and lim, windows of vref, history = 82 > max_iter: for all 230 starts the cost,
    the iteration count, the count of entries and the eight fields the driver's trace records (lambda g_norm dV0 dV1 cost
    new_cost alpha_idx bp_calls) equal Driver.solve() / Driver.trace() under that start's own parameter dict and window, bit
    for bit.  The driver records neither z nor the penalty weights nor the iteration index: the index must count 0 .. n - 1,
    z must be line_search.c's ratio of the recorded fields where a step was accepted, and all three are held bit for bit, every
    entry, to the plain solves' history (which tests/test_gpu_history.py holds to polled fields)."""
    name, cap = "almix_strict", 82
    inp = inputs(name)
    got = streamed(ilqg, name, history=cap)
    h = got["history"]
    unwritten_are_zero(h, name)
    lib = lib_path("oracle", inp.problem, inp.fd)
    for s in range(TOTAL):
        ref = oracle_solve(lib, inp, s, trace=True)
        assert ref["init"] == 1 and got["status"][s] != 7, s
        assert got["cost"][s] == ref["cost"] and got["iterations"][s] == ref["iterations"], (s, got["cost"][s], ref["cost"], got["iterations"][s], ref["iterations"])
        mine, tr = valid(h, s), ref["trace"]
        n = int(h["n"][s])
        assert n == len(tr["lambda"]) <= cap, (s, n, len(tr["lambda"]))
        for k in TRACE:
            assert np.array_equal(mine[k], tr[k]), (s, k)
        assert np.array_equal(mine["iterations"], np.arange(n)), s
        acc = mine["alpha_idx"] <= len(DEFAULT_ALPHA)
        alpha = np.asarray(DEFAULT_ALPHA)[np.minimum(mine["alpha_idx"], len(DEFAULT_ALPHA)) - 1]
        assert np.array_equal(mine["z"][acc], z_recipe(mine["cost"], mine["new_cost"], alpha, mine["dV0"], mine["dV1"])[2][acc]), s
    want = plain(ilqg, name, history=cap)
    results_equal(got, want, name)
    histories_equal(h, want["history"], name)
    assert len(np.unique(h["n"])) >= 4


# ---------------------------------------------------------------------------
# 3. a history per start
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("name,batch,total,cap", [("hxtest", B, TOTAL, 48), ("hxtest", B, TOTAL, 5), ("synth16x8", 8, 27, 122), ("synth16x8", 8, 27, 3)])
def test_the_streams_history_is_the_plain_solves_history(ilqg, name, batch, total, cap):
    """every field, every position and the counts, with a capacity beyond the longest solve and with one below it (dropped but
    counted); hxtest under its rows, synth16x8 (wave mapping: a history alone) without"""
    got, want = streamed(ilqg, name, history=cap, total=total, batch=batch), plain(ilqg, name, history=cap, total=total)
    results_equal(got, want, name)
    histories_equal(got["history"], want["history"], "%s cap %d" % (name, cap))
    unwritten_are_zero(got["history"], name)
    n = got["history"]["n"]
    assert (n.max() > cap) == (cap <= 5) and len(np.unique(n)) >= 2, (cap, np.unique(n))
    assert got["trace"][3] >= 4


def raw_args(inp, total, rows=True, hist_cap=0, hist_names=(), trajectories=False):
    """the arguments of ilqg_batch_solve_stream_rows for the first `total` starts, by name"""
    rows = rows and has_rows(inp)
    names = list(inp.rows) if rows else []
    a = dict(total=total, x0=np.ascontiguousarray(inp.x0[:total]), u0=np.ascontiguousarray(inp.u0[:total]), names=names,
             values=np.ascontiguousarray(np.concatenate([inp.rows[n][:total].reshape(total, -1) for n in names], axis=1)) if names else None,
             step_names=list(inp.steps) if rows else [], step_values=[np.ascontiguousarray(t[:total]) for t in inp.steps.values()] if rows else [],
             hist_cap=hist_cap, hist_names=list(hist_names),
             hist_out=[np.full(total if n == "n" else (total, max(hist_cap, 1)), -7, dtype=np.int32 if n in ("n", "alpha_idx", "bp_calls", "iterations") else np.float64)
                       for n in hist_names],
             cost=np.full(total, -7.0), status=np.full(total, -7, dtype=np.int32), iterations=np.full(total, -7, dtype=np.int32),
             x=np.full((total, inp.N + 1, inp.x0.shape[1]), -7.0) if trajectories else None,
             u=np.full((total, inp.N, inp.u0.shape[2]), -7.0) if trajectories else None)
    return a


def raw_call(s, a, **over):
    """the C entry itself; over: arguments replaced, or counts given on their own (n_names, n_step_names, n_hist).  Returns
    (rc, error text, the arguments)"""
    a = dict(a, **over)
    strings = lambda l: None if l is None else (C.c_char_p * len(l))(*[None if n is None else n.encode() for n in l])
    ptrs = lambda l: None if l is None else (C.c_void_p * len(l))(*[None if v is None else v.ctypes.data for v in l])
    addr = lambda v: None if v is None else v.ctypes.data_as(C.c_void_p)
    count = lambda key, of: a[key] if key in a else (0 if a[of] is None else len(a[of]))
    rc = s.lib.ilqg_batch_solve_stream_rows(s.h, a["total"], addr(a["x0"]), addr(a["u0"]), count("n_names", "names"), strings(a["names"]), addr(a["values"]),
                                            count("n_step_names", "step_names"), strings(a["step_names"]), ptrs(a["step_values"]),
                                            a["hist_cap"], count("n_hist", "hist_names"), strings(a["hist_names"]), ptrs(a["hist_out"]),
                                            addr(a["cost"]), addr(a["status"]), addr(a["iterations"]), addr(a["x"]), addr(a["u"]))
    return rc, s.lib.ilqg_batch_error(s.h).decode(), a


def test_a_subset_of_the_history_names(ilqg):
    """the C entry with three of the names, in an order of the caller's: each array is the full history's field"""
    name, cap, pick = "hxtest", 48, ("n", "lambda", "alpha_idx")
    inp, full = inputs(name), streamed(ilqg, name, history=cap)
    s = make(ilqg, inp, B)
    rc, err, a = raw_call(s, raw_args(inp, TOTAL, hist_cap=cap, hist_names=pick))
    s.close()
    assert rc == 0, err
    for k, out in zip(pick, a["hist_out"]):
        assert out.dtype == full["history"][k].dtype and np.array_equal(out, full["history"][k]), k
    results_equal(a, full, name, keys=("cost", "status", "iterations"))


# ---------------------------------------------------------------------------
# 4. the old entry through the one loop
# ---------------------------------------------------------------------------
def test_the_old_entry_is_the_new_one_with_nothing_named(ilqg):
    """FMA-free CarParking: solve_stream(x0, u0) (ilqg_batch_solve_stream), solve_stream(params={}) (the new entry, nothing
    named) and a table of the shared values per start give the same bits; a poll in which nothing finished launches no
    k_harvest, every start is copied to the host once, and no context is made but the staging context"""
    name = "carparking_strict"
    inp = inputs(name)
    s = make(ilqg, inp, B, groups=1)
    s.timing(True)
    old = s.solve_stream(inp.x0, inp.u0, with_trajectories=True)
    trace, counts, timed = s.solve_trace(), s.stream_counts(), launches(s)
    s.close()
    # the new entry with nothing named: params = {} is given to solve_stream itself, which then calls
    # ilqg_batch_solve_stream_rows with n_names = n_step_names = hist_cap = 0 (tests/test_solve_stream_rows_binding.py holds
    # that routing); a solver of its own, made like the first
    s = make(ilqg, inp, B, groups=1)
    new = s.solve_stream(inp.x0, inp.u0, with_trajectories=True, params={})
    new["trace"], new["counts"] = s.solve_trace(), s.stream_counts()
    s.close()
    results_equal(old, new, "params = {}")
    assert "history" not in old and "history" not in new
    assert len(trace) == len(new["trace"]) == 4
    for a, b in zip(trace, new["trace"]):
        assert np.array_equal(a, b)
    s = make(ilqg, inp, B)
    nominal = run_stream(s, inp, table=inp.nominal_rows())
    s.close()
    results_equal(nominal, old, "a table of the shared values")
    # polls at fewer iterations than the shortest solve find nothing finished: the first of them finds nothing started
    polls, words = len(trace[0]), 2 + (inp.N + 1) * inp.x0.shape[1] + inp.N * inp.u0.shape[2]
    quiet = (int(old["iterations"].min()) - 1) // 8 + 1
    assert counts["polls"] == polls and quiet >= 2
    assert 1 <= counts["harvests"] <= polls - quiet, (counts, polls, quiet)
    assert timed["layout kernels"] == counts["harvests"], (timed["layout kernels"], counts)  # (k_harvest is timed as a layout kernel)
    assert counts["harvest_bytes"] == TOTAL * words * 8 and counts["contexts"] == 1, counts
    assert new["counts"] == counts


# ---------------------------------------------------------------------------
# 5. identities, bit for bit
# ---------------------------------------------------------------------------
def test_the_starts_reversed_give_the_results_reversed(ilqg):
    name, cap = "hxtest", 48
    inp, want = inputs(name), streamed(ilqg, name, history=cap)
    s = make(ilqg, inp, B)
    got = run_stream(s, inp, sel=slice(None, None, -1), history=cap)
    s.close()
    results_equal(got, want, "reversed", rows_want=slice(None, None, -1))
    histories_equal(got["history"], want["history"], "reversed", rows_b=slice(None, None, -1))


def test_names_in_another_order_and_an_extra_nominal_name(ilqg):
    name = "hxtest"
    inp, want = inputs(name), streamed(ilqg, name)
    s = make(ilqg, inp, B)
    swapped = run_stream(s, inp, table={n: inp.rows[n] for n in reversed(list(inp.rows))})
    extra = [n for n in inp.params if n not in inp.rows and n != "h"][0]
    more = dict(inp.rows)
    more[extra] = np.ascontiguousarray(np.broadcast_to(inp.params[extra], (TOTAL, inp.params[extra].size)))
    added = run_stream(s, inp, table=more)
    s.close()
    results_equal(swapped, want, "names reversed, columns with them")
    results_equal(added, want, "a nominal column of '%s'" % extra)


@pytest.mark.parametrize("groups,batch", [(1, B), (2, B), (4, 200), (0, 8)])
def test_groups_and_batch_sizes(ilqg, groups, batch):
    """1, 2 and 4 stream groups (a group is whole tiles of 64 slots: four need 200), and B = 8: fewer than 16 slots, the
    refill threshold is 0"""
    name, cap = "almix", 82
    inp, want = inputs(name), streamed(ilqg, name, history=cap)
    s = make(ilqg, inp, batch, groups=groups)
    assert groups == 0 or s.groups() == groups
    got = run_stream(s, inp, history=cap)
    s.close()
    results_equal(got, want, "groups %d, B %d" % (groups, batch))
    histories_equal(got["history"], want["history"], "groups %d, B %d" % (groups, batch))
    assert np.all(got["trace"][2] == batch)


@pytest.mark.parametrize("total", [40, 1])
def test_fewer_starts_than_slots(ilqg, total):
    name, cap = "almix", 82
    inp, want = inputs(name), streamed(ilqg, name, history=cap)
    s = make(ilqg, inp, B)
    got = run_stream(s, inp, sel=slice(0, total), history=cap)
    s.close()
    results_equal(got, want, "total %d" % total, rows_want=slice(0, total))
    histories_equal(got["history"], want["history"], "total %d" % total, rows_b=slice(0, total))
    assert got["trace"][3] == 1


# ---------------------------------------------------------------------------
# 6. failure is per start
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("what", ["window", "x0"])
def test_a_start_that_cannot_initialise_fails_alone(ilqg, what):
    """a NaN time step in one start's window, or a NaN x0: status 7 for that start, no other start changed by a bit"""
    name, cap, bad = "almix", 82, 77
    want = streamed(ilqg, name, history=cap)
    inp = Inputs(name)  # (a copy of its own: the shared inputs stay as they are)
    if what == "window":
        inp.steps["vref"][bad, 11] = np.nan
    else:
        inp.x0[bad, 1] = np.nan
    s = make(ilqg, inp, B)
    got = run_stream(s, inp, history=cap)
    s.close()
    assert got["status"][bad] == 7 and want["status"][bad] != 7 and got["history"]["n"][bad] == 0
    others = np.arange(TOTAL) != bad
    results_equal(got, want, what, rows_got=others, rows_want=others)
    histories_equal(got["history"], want["history"], what, rows_a=others, rows_b=others)


# ---------------------------------------------------------------------------
# 7. nothing is left behind
# ---------------------------------------------------------------------------
def after_a_stream(s, inp, fresh_state):
    for n in inp.rows:
        assert np.array_equal(s.params_batch(n), np.broadcast_to(inp.params[n], (B, inp.params[n].size))), n
    for n in inp.steps:
        assert np.array_equal(s.param_steps_batch(n), np.broadcast_to(inp.params[n], (B, inp.N + 1))), n
    assert s.lib.ilqg_batch_history_cap(s.h) == 0
    s.init(inp.x0[:B], inp.u0[:B])
    s.solve()
    assert_state_equal(full_state(s), fresh_state, "init + solve behind a stream")


def test_nothing_is_left_behind(ilqg):
    """after a stream with all three payloads, and after a refused call: the shared values, no history, and an init + solve
    that equals a fresh solver's in full_state of tests/test_gpu_receding_plant.py — x, u, gains, cost, status, iterations,
    lambda, multipliers and penalty weights.  (The per-step-size costs of the LAST line search are left out: init() does not
    clear them, and a search writes those of the step sizes it rolls out only, so behind any earlier solve the others hold
    what that solve left, as they do between two plain solves.)"""
    name = "almix"
    inp = inputs(name)
    fresh = make(ilqg, inp, B)
    fresh.init(inp.x0[:B], inp.u0[:B])
    fresh.solve()
    fresh_state = full_state(fresh)
    fresh.close()
    s = make(ilqg, inp, B)
    run_stream(s, inp, history=82)
    after_a_stream(s, inp, fresh_state)
    rc, err, _ = raw_call(s, raw_args(inp, TOTAL, hist_cap=4, hist_names=("n", "nope")))
    assert rc != 0 and "nope" in err
    after_a_stream(s, inp, fresh_state)
    s.close()


# ---------------------------------------------------------------------------
# 8. refusals
# ---------------------------------------------------------------------------
def refusals_of(inp, s, a):
    """(call, words) of every refusal of include/ilqg_batch.h this build can show"""
    names, steps = a["names"], a["step_names"]
    out = [(lambda: raw_call(s, a, total=0), ("total = 0",)), (lambda: raw_call(s, a, total=-3), ("total = -3",)),
           (lambda: raw_call(s, a, x0=None), ("x0 is NULL",)), (lambda: raw_call(s, a, u0=None), ("u0 is NULL",)),
           (lambda: raw_call(s, a, hist_cap=-1), ("hist_cap = -1",)),
           (lambda: raw_call(s, a, hist_cap=0, hist_names=["n"], hist_out=[a["status"]]), ("n_hist = 1", "hist_cap = 0")),
           (lambda: raw_call(s, a, hist_cap=4, hist_names=["n", "nope"], hist_out=[a["status"], a["status"]]), ("hist_names[1]", "no such history field 'nope'")),
           (lambda: raw_call(s, a, hist_cap=4, hist_names=["n", "z"], hist_out=[a["status"], None]), ("hist_out[1] is NULL", "'z'")),
           (lambda: raw_call(s, a, hist_cap=4, hist_names=["n"], hist_out=None), ("hist_out is NULL",))]
    if not sum(s.multiplier_dims()):
        out.append((lambda: raw_call(s, a, hist_cap=4, hist_names=["w_pen_l"], hist_out=[a["cost"]]), ("hist_names[0]", "w_pen_l", "multipliers only")))
    if not has_rows(inp):
        some = [n for n, size in s.problem.params if size > 0][0]
        table = np.zeros((a["total"], dict(s.problem.params)[some]))
        out.append((lambda: raw_call(s, a, names=[some], values=table), ("wave mapping", "lane-mapped")))
        out.append((lambda: raw_call(s, a, step_names=["vref"], step_values=[table]), ("wave mapping",)))
        return out
    out += [(lambda: raw_call(s, a, n_names=-1), ("n_names = -1",)), (lambda: raw_call(s, a, names=None, n_names=len(names)), ("names is NULL",)),
            (lambda: raw_call(s, a, values=None), ("values is NULL",)),
            (lambda: raw_call(s, a, names=names[:-1] + ["nope"]), ("names[%d]" % (len(names) - 1), "Parameter name 'nope' is not member of parameters struct.")),
            (lambda: raw_call(s, a, names=names[:-1] + [names[0]]), ("names[%d]" % (len(names) - 1), "'%s'" % names[0], "twice")),
            (lambda: raw_call(s, a, step_names=[names[0]], step_values=[a["values"]]), ("step_names[0]", "'%s'" % names[0], "fixed size")),
            (lambda: raw_call(s, a, step_names=["nope"], step_values=[a["values"]]), ("step_names[0]", "Parameter name 'nope' is not member of parameters struct.")),
            (lambda: raw_call(s, a, step_names=[None], step_values=[a["values"]]), ("step_names[0]", "NULL"))]
    if steps:
        out += [(lambda: raw_call(s, a, names=names[:-1] + [steps[0]]), ("names[%d]" % (len(names) - 1), "'%s'" % steps[0], "per time step")),
                (lambda: raw_call(s, a, step_names=steps + steps, step_values=a["step_values"] * 2), ("step_names[1]", "'%s'" % steps[0], "twice")),
                (lambda: raw_call(s, a, step_values=[None]), ("step_values[0] is NULL", "'%s'" % steps[0])),
                (lambda: raw_call(s, a, step_values=None), ("step_values is NULL",))]
    return out


@pytest.mark.parametrize("name", ["almix", "hxtest", "carparking_wave", "synth16x8"])
def test_refusals(ilqg, name):
    """every refusal names the entry and the argument, writes no output, launches nothing and leaves the batch's trajectories
    those of a twin that was never called"""
    total = 12
    inp = inputs(name, TOTAL if has_rows(inputs(name)) else 27)
    batch = B if has_rows(inp) else 8
    s, twin = make(ilqg, inp, batch), make(ilqg, inp, batch)
    for q in (s, twin):
        q.init(inp.x0[:batch], inp.u0[:batch])
        q.iterate(3)
    s.timing(True)
    a = raw_args(inp, total, trajectories=True)
    calls = refusals_of(inp, s, a)
    if has_rows(inp):  # a batch that already has a set, rows or a history: the text tells the caller to pass them to this call
        def with_state(put, clear, *words):
            def call():
                put()
                try:
                    return raw_call(s, a)
                finally:
                    clear()
            return call, ("c: the batch already",) + words
        calls.append(with_state(lambda: s.set_params_batch({n: t[:batch] for n, t in inp.rows.items()}), lambda: s.set_params_batch(None),
                                "ilqg_batch_set_params_batch", "names, values"))
        calls.append(with_state(lambda: s.set_history(6), lambda: s.set_history(0), "ilqg_batch_set_history", "hist_cap"))
        for n, t in inp.steps.items():
            calls.append(with_state(lambda n=n, t=t: s.set_param_steps_batch(n, t[:batch]), lambda n=n: s.set_param_steps_batch(n, None),
                                    "ilqg_batch_set_param_steps_batch", "step_names, step_values", "'%s'" % n))
    for call, words in calls:
        rc, err, _ = call()
        assert rc != 0, words
        for w in ("ilqg_batch_solve_stream_rows",) + tuple(words):
            assert w in err, (w, err)
    assert all(np.all(a[k] == -7) for k in ("cost", "status", "iterations", "x", "u")), "a refused call wrote an output"
    ran = {k: n for k, n in launches(s).items() if n}
    assert not ran, ran
    assert_state_equal(full_state(s), full_state(twin), "%s behind refused calls" % name)
    s.close()
    twin.close()


def test_the_python_keywords_are_checked_before_the_library(ilqg):
    inp = inputs("hxtest")
    s = make(ilqg, inp, B)
    for kw, words in ((dict(history=-1), ("history = -1",)), (dict(history=2.5), ("history", "integer")), (dict(params=[1]), ("params", "dict")),
                      (dict(params={"nope": np.zeros(TOTAL)}), ("Parameter name 'nope'",)),
                      (dict(params={"cf": np.zeros((TOTAL - 1, 3))}), ("params['cf']", "shape")),
                      (dict(param_steps={"cf": np.zeros((TOTAL, inp.N + 1))}), ("'cf'", "fixed size"))):
        with pytest.raises(ilqg.IlqgError) as e:
            s.solve_stream(inp.x0, inp.u0, **kw)
        for w in ("solve_stream",) + words:
            assert w in str(e.value), (w, str(e.value))
    s.close()
