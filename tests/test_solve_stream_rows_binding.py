"""ilqg.py's side of BatchSolver.solve_stream(params=..., param_steps=..., history=...), where no GPU is needed: without the
new keywords the call goes to ilqg_batch_solve_stream with the arguments it has always had; with one of them it goes to
ilqg_batch_solve_stream_rows with the rows packed [total, W] in dict order, one table [total, n_hor+1] per per-time-step
name, and one output array per history name of the library's problem — doubles [total, cap] float64, ints [total, cap] int32,
"n" [total]; bad arguments are refused before any library call; a library built before the entry existed says "rebuild"; and
the public header declares the entry, states its refusals and the "as on entry" rule.  Modelled on
tests/test_history_binding.py."""
import ctypes as C
import os
import re
import types

import numpy as np
import pytest

from conftest import ROOT, load_package
from history_cases import DOUBLES, INTS, PENALTIES

B, N, NX, NU, TOTAL, CAP = 5, 12, 4, 2, 9, 7
PARAMS = [("h", 1), ("cf", 3), ("lim", 2), ("vref", -1), ("wref", -1)]


def array(ptr, ctype, shape):
    return np.ctypeslib.as_array(C.cast(ptr, C.POINTER(ctype)), shape=shape)


class OldLibrary:
    """stands for a CDLL without the new symbol: the old entry records its call"""

    def __init__(self):
        self.calls = []
        self.ilqg_batch_solve_stream = self._old()  # (a plain function on the instance: the wrapper sets .argtypes on it)

    def _old(self):
        def old(h, total, x0, u0, cost, status, iters, x, u):
            self.calls.append(("ilqg_batch_solve_stream", total, x0.copy(), u0.copy(), x is not None, u is not None))
            cost[:], status[:], iters[:] = np.arange(total) + 0.5, 2, np.arange(total)
            return 0
        return old

    def ilqg_problem_multiplier_dims(self, d):
        d[:] = 0


class Recorder(OldLibrary):
    """stands for a library that has it: remembers what the entry was called with and fills the outputs with ramps"""

    def __init__(self, multipliers=(0, 0)):
        super().__init__()
        self.multipliers = multipliers
        self.ilqg_batch_solve_stream_rows = self._rows()

    def ilqg_problem_multiplier_dims(self, d):
        d[:] = self.multipliers

    def _rows(self):
        def rows(h, total, x0, u0, n_names, names, values, n_step, step_names, step_values, cap, n_hist, hist_names, hist_out,
                 cost, status, iters, x, u):
            for v in (total, n_names, n_step, cap, n_hist):
                assert type(v) is int
            call = dict(total=total, x0=array(x0, C.c_double, (total, NX)).copy(), u0=array(u0, C.c_double, (total, N, NU)).copy(),
                        names=[names[i].decode() for i in range(n_names)], step_names=[step_names[i].decode() for i in range(n_step)],
                        cap=cap, hist_names=[hist_names[i].decode() for i in range(n_hist)], x=x is not None, u=u is not None)
            W = sum(dict(PARAMS)[n] for n in call["names"])
            call["values"] = array(values, C.c_double, (total, W)).copy() if n_names else values
            call["step_values"] = [array(step_values[i], C.c_double, (total, N + 1)).copy() for i in range(n_step)]
            for i, name in enumerate(call["hist_names"]):
                is_int = name in INTS + ("n",)
                count = total if name == "n" else total * cap
                array(hist_out[i], C.c_int if is_int else C.c_double, (count,))[:] = np.arange(count) + i
            array(cost, C.c_double, (total,))[:] = np.arange(total) + 0.5
            array(status, C.c_int, (total,))[:] = 2
            array(iters, C.c_int, (total,))[:] = np.arange(total)
            self.calls.append(("ilqg_batch_solve_stream_rows", call))
            return 0
        return rows


def solver(ilqg, lib):
    s = object.__new__(ilqg.BatchSolver)
    s.lib, s.h, s.B, s.N, s.device = lib, 1, B, N, 0
    s.problem = types.SimpleNamespace(nx=NX, nu=NU, params=PARAMS)
    return s


@pytest.fixture(scope="module")
def ilqg():
    return load_package().ilqg


def starts():
    rng = np.random.default_rng(5)
    return rng.standard_normal((TOTAL, NX)), rng.standard_normal((TOTAL, N, NU))


def test_without_the_new_keywords_the_old_entry_is_called(ilqg):
    x0, u0 = starts()
    for lib in (OldLibrary(), Recorder()):
        s = solver(ilqg, lib)
        out = s.solve_stream(x0, u0)
        out2 = s.solve_stream(x0, u0, with_trajectories=True)
        assert [c[0] for c in lib.calls] == ["ilqg_batch_solve_stream"] * 2
        assert lib.calls[0][1] == TOTAL and np.array_equal(lib.calls[0][2], x0) and np.array_equal(lib.calls[0][3], u0)
        assert lib.calls[0][4:] == (False, False) and lib.calls[1][4:] == (True, True)
        assert set(out) == {"cost", "status", "iterations", "x", "u"} and out["x"] is None and out2["x"].shape == (TOTAL, N + 1, NX)
        assert out["status"].dtype == np.int32 and np.array_equal(out["iterations"], np.arange(TOTAL))


def test_the_new_keywords_on_an_old_library_say_rebuild(ilqg):
    x0, u0 = starts()
    lib = OldLibrary()
    s = solver(ilqg, lib)
    for kw in (dict(params={"cf": np.zeros((TOTAL, 3))}), dict(param_steps={"vref": np.zeros((TOTAL, N + 1))}), dict(history=4), dict(params={})):
        with pytest.raises(ilqg.IlqgError) as e:
            s.solve_stream(x0, u0, **kw)
        assert "ilqg_batch_solve_stream_rows" in str(e.value) and "rebuild" in str(e.value), str(e.value)
    assert lib.calls == []


@pytest.mark.parametrize("multipliers", [(0, 0), (3, 2)])
def test_rows_windows_and_history_are_marshalled(ilqg, multipliers):
    x0, u0 = starts()
    lib = Recorder(multipliers)
    s = solver(ilqg, lib)
    rng = np.random.default_rng(9)
    cf, h, lim = rng.standard_normal((TOTAL, 3)), rng.standard_normal(TOTAL), rng.standard_normal((TOTAL, 2))
    vref, wref = rng.standard_normal((TOTAL, N + 1)), rng.standard_normal((TOTAL, N + 1))
    # float32, strided and Fortran-ordered arguments arrive as C-contiguous doubles; the last axis may be left out for size 1
    out = s.solve_stream(x0, u0, with_trajectories=True, params={"lim": np.asfortranarray(lim), "h": h.astype(np.float32), "cf": cf},
                         param_steps={"wref": wref[:, ::1], "vref": np.asfortranarray(vref)}, history=np.int64(CAP))
    (entry, call), = lib.calls
    assert entry == "ilqg_batch_solve_stream_rows" and call["total"] == TOTAL and call["x"] and call["u"]
    assert np.array_equal(call["x0"], x0) and np.array_equal(call["u0"], u0)
    assert call["names"] == ["lim", "h", "cf"]
    assert np.array_equal(call["values"], np.concatenate([lim, h.astype(np.float32).astype(np.float64)[:, None], cf], axis=1))
    assert call["step_names"] == ["wref", "vref"] and np.array_equal(call["step_values"][0], wref) and np.array_equal(call["step_values"][1], vref)
    doubles = DOUBLES + (PENALTIES if sum(multipliers) else ())
    assert call["cap"] == CAP and call["hist_names"] == list(doubles + INTS + ("n",))
    hist = out["history"]
    assert list(hist) == call["hist_names"]
    for i, k in enumerate(hist):
        if k == "n":
            assert hist[k].shape == (TOTAL,) and hist[k].dtype == np.int32
        else:
            assert hist[k].shape == (TOTAL, CAP) and hist[k].dtype == (np.int32 if k in INTS else np.float64), k
        assert np.array_equal(hist[k].reshape(-1), np.arange(hist[k].size) + i), k
    assert np.array_equal(out["cost"], np.arange(TOTAL) + 0.5) and out["status"].dtype == np.int32 and out["x"].shape == (TOTAL, N + 1, NX)
    # each payload alone, and none: n = 0 and NULL for what is not given; no `history` in the result without a capacity
    lib.calls.clear()
    for kw in (dict(params={"cf": cf}), dict(param_steps={"vref": vref}), dict(history=3), dict(params={}), dict(param_steps={}, params=None)):
        out = s.solve_stream(x0, u0, **kw)
        call = lib.calls[-1][1]
        assert call["names"] == list(kw.get("params") or {}) and call["step_names"] == list(kw.get("param_steps") or {})
        assert call["cap"] == kw.get("history", 0) and (call["hist_names"] != []) == ("history" in kw) == ("history" in out)
        assert not call["x"] and not call["u"] and (call["names"] or call["values"] is None)
    assert [c[0] for c in lib.calls] == ["ilqg_batch_solve_stream_rows"] * 5


def test_bad_arguments_are_refused_before_any_library_call(ilqg):
    x0, u0 = starts()
    lib = Recorder()
    s = solver(ilqg, lib)
    ok = np.zeros((TOTAL, N + 1))
    for kw, words in ((dict(history=-1), ("history = -1", "negative")), (dict(history=2.0), ("history", "integer")), (dict(history=True), ("history", "integer")),
                      (dict(history="3"), ("history", "integer")), (dict(params=[("cf", 1)]), ("params", "dict")), (dict(param_steps=ok), ("param_steps", "dict")),
                      (dict(params={"nope": np.zeros(TOTAL)}), ("params", "Parameter name 'nope' is not member of parameters struct.")),
                      (dict(params={"vref": ok}), ("params", "'vref'", "per time step")),
                      (dict(params={"cf": np.zeros((B, 3))}), ("params['cf']", "shape (5, 3)", "(9, 3)", "total = 9")),
                      (dict(params={"cf": np.zeros(TOTAL)}), ("params['cf']", "shape")),
                      (dict(param_steps={"cf": ok}), ("name", "'cf'", "fixed size of 3")),
                      (dict(param_steps={"nope": ok}), ("Parameter name 'nope' is not member of parameters struct.",)),
                      (dict(param_steps={"vref": np.zeros((TOTAL, N))}), ("param_steps['vref']", "shape (9, 12)", "(9, 13)"))):
        with pytest.raises(ilqg.IlqgError) as e:
            s.solve_stream(x0, u0, **kw)
        for w in ("solve_stream",) + words:
            assert w in str(e.value), (w, str(e.value))
    assert lib.calls == []


def test_the_header_declares_the_entry_and_states_its_rules():
    text = open(os.path.join(ROOT, "include", "ilqg_batch.h")).read()
    flat = " ".join(text.replace("\n *", " ").split())
    m = re.search(r"int ilqg_batch_solve_stream_rows\((.*?)\);", text, re.S)
    assert m, "ilqg_batch_solve_stream_rows is not declared"
    args = " ".join(m.group(1).split())
    assert args == ("ilqg_batch_t *c, int total, const double *x0, const double *u0, int n_names, const char *const *names, const double *values, "
                    "int n_step_names, const char *const *step_names, const double *const *step_values, int hist_cap, int n_hist, "
                    "const char *const *hist_names, void *const *hist_out, double *cost, int *status, int *iterations, double *x, double *u")
    for words in ("ilqg_batch_solve_stream is this entry with nothing named",
                  "the plain solve's result bit for bit, in every build",
                  "values [total][W]", "step_values[i] [total][n_hor+1]",
                  "double [total][hist_cap] for a double name, int [total][hist_cap] for an int name and int [total] for \"n\"",
                  "n may exceed hist_cap",
                  "on return, success or failure, c is as on entry",
                  "ilqg_batch_history_cap gives 0",
                  "before anything is launched, allocated or changed",
                  "one launch and one copy",
                  "No context is made per poll"):
        assert words in flat, words
    for refusal in ("total < 1", "x0 or u0 NULL", "a c that already has a set, rows or a history", "pass them to this call",
                    "what ilqg_batch_set_params_batch refuses of names / values", "fixed-size, unknown, given twice, a NULL table",
                    "hist_cap < 0", "n_hist > 0 with hist_cap = 0", "an unknown history name", "w_pen_* without multipliers", "a NULL hist_out[i]",
                    "n_names > 0 or n_step_names > 0 (the text names the mapping)", "a history alone is served there"):
        assert refusal in flat, refusal
    # the three notes of the existing entry stay and point at the new one
    assert flat.count("ilqg_batch_solve_stream_rows") >= 5
    ilqg = load_package().ilqg
    doc = " ".join(ilqg.BatchSolver.solve_stream.__doc__.split())
    assert "ilqg_batch_solve_stream_rows" in doc and "[total, n_hor+1]" in doc and "has none afterwards" in doc and "rebuild" in doc


def test_the_host_states_the_loop_once():
    """ilqg_batch_solve_stream keeps its three refusals with their texts, in front, and is the new entry with nothing named"""
    host = open(os.path.join(ROOT, "ddp-generator_amd", "csrc", "ilqg_host.c")).read()
    old = re.search(r"\nint ilqg_batch_solve_stream\(.*?\n}\n", host, re.S).group(0)
    joined = re.sub(r'"\s*"', "", old)  # (adjacent string literals as the compiler joins them)
    for words in ("a table per start is not supported", "rows per start are not supported", "a history per start is not supported"):
        assert words in joined, words
    assert joined.index("no starts") < joined.index("a table per start") < joined.index("rows per start") < joined.index("a history per start") < joined.index("return ilqg_batch_solve_stream_rows")
    assert "return ilqg_batch_solve_stream_rows(c, total, x0, u0, 0, NULL, NULL, 0, NULL, NULL, 0, 0, NULL, NULL, cost, status, iterations, x, u);" in old
    assert "iterate_groups" not in old and host.count("iterate_groups(c, ILQG_STREAM_ROUND)") == 1
    assert "working_copy(c, m)" not in host.split("static int stream_solve")[1].split("int ilqg_batch_solve_trace")[0]
