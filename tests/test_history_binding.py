"""ilqg.py's side of BatchSolver.set_history / history and MultiSolver's twins, where no GPU is needed: the capacity reaches
ilqg_batch_set_history / ilqg_multi_set_history as an int; history() asks every name of the library once — the doubles through
ilqg_batch_get_history into [B, cap] float64, the ints through ilqg_batch_get_history_int into [B, cap] int32, "n" into [B] —
and w_pen_* only where the library's problem has multipliers; bad arguments are refused before any library call; a library built
before the entries existed says "rebuild"; and the public header declares the entries and states the one rule.  Modelled on
tests/test_params_batch_binding.py."""
import ctypes as C
import os
import re
import types

import numpy as np
import pytest

from conftest import ROOT, load_package
from history_cases import DEFAULT_ALPHA, DOUBLES, INTS, PENALTIES

B, N, NX, NU, CAP = 5, 12, 4, 2, 7
BATCH = ["ilqg_batch_set_history", "ilqg_batch_get_history", "ilqg_batch_get_history_int", "ilqg_batch_history_cap"]
MULTI = ["ilqg_multi_set_history", "ilqg_multi_get_history", "ilqg_multi_get_history_int", "ilqg_multi_history_cap"]


class OldLibrary:
    """stands for a CDLL without the new symbols"""

    def ilqg_problem_multiplier_dims(self, d):
        d[:] = 0


class Recorder:
    """stands for a library that has them: remembers what each entry was called with and fills the outputs with a ramp"""

    def __init__(self, multipliers=(0, 0), cap=CAP):
        self.calls, self.multipliers, self.cap = [], multipliers, cap
        for names in (BATCH, MULTI):
            setattr(self, names[0], self._set(names[0]))
            setattr(self, names[1], self._get(names[1], C.c_double))
            setattr(self, names[2], self._get(names[2], C.c_int))
            setattr(self, names[3], lambda h: self.cap)

    def ilqg_problem_multiplier_dims(self, d):
        d[:] = self.multipliers

    def _set(self, entry):
        def call(h, cap):
            assert type(cap) is int
            self.calls.append((entry, cap))
            self.cap = cap
            return 0
        return call

    def _get(self, entry, ctype):
        def call(h, name, out):
            name = name.decode()
            count = B if name == "n" else B * self.cap
            a = np.ctypeslib.as_array(C.cast(out, C.POINTER(ctype)), shape=(count,))
            a[:] = np.arange(count)
            self.calls.append((entry, name))
            return 0
        return call


def solver(ilqg, lib, cls=None):
    s = object.__new__(cls or ilqg.BatchSolver)
    s.lib, s.h, s.B, s.N, s.device = lib, 1, B, N, 0
    s.problem = types.SimpleNamespace(nx=NX, nu=NU, params=[])
    return s


@pytest.fixture(scope="module")
def ilqg():
    return load_package().ilqg


def test_the_capacity_reaches_the_entry(ilqg):
    lib = Recorder()
    s, m = solver(ilqg, lib), solver(ilqg, lib, ilqg.MultiSolver)
    s.set_history(32)
    s.set_history(np.int64(3))
    s.set_history(0)
    m.set_history(4)
    assert lib.calls == [(BATCH[0], 32), (BATCH[0], 3), (BATCH[0], 0), (MULTI[0], 4)]


@pytest.mark.parametrize("multipliers", [(0, 0), (6, 6), (0, 2)])
def test_history_asks_every_name_once_and_returns_the_documented_shapes(ilqg, multipliers):
    for cls, names in ((None, BATCH), ("multi", MULTI)):
        lib = Recorder(multipliers)
        s = solver(ilqg, lib, ilqg.MultiSolver if cls else None)
        h = s.history()
        doubles = DOUBLES + (PENALTIES if sum(multipliers) else ())
        assert list(h) == list(doubles + INTS + ("n",))
        assert lib.calls == [(names[1], k) for k in doubles] + [(names[2], k) for k in INTS + ("n",)]
        for k in doubles:
            assert h[k].shape == (B, CAP) and h[k].dtype == np.float64 and np.array_equal(h[k].reshape(-1), np.arange(B * CAP)), k
        for k in INTS:
            assert h[k].shape == (B, CAP) and h[k].dtype == np.int32 and np.array_equal(h[k].reshape(-1), np.arange(B * CAP)), k
        assert h["n"].shape == (B,) and h["n"].dtype == np.int32 and np.array_equal(h["n"], np.arange(B))
        lib.calls.clear()
        assert list(s.history("z")) == ["z"] and list(s.history(("n", "lambda"))) == ["n", "lambda"]
        assert lib.calls == [(names[1], "z"), (names[2], "n"), (names[1], "lambda")]


def test_bad_arguments_are_refused_before_any_library_call(ilqg):
    lib = Recorder()
    s, m = solver(ilqg, lib), solver(ilqg, lib, ilqg.MultiSolver)
    for q in (s, m):
        for cap, words in ((-1, ("set_history", "cap = -1", "negative")), (2.0, ("set_history", "integer")), (True, ("set_history", "integer")),
                           ("3", ("set_history", "integer")), (None, ("set_history", "integer"))):
            with pytest.raises(ilqg.IlqgError) as e:
                q.set_history(cap)
            assert all(w in str(e.value) for w in words), str(e.value)
        for names, words in (("nope", ("history", "no such history field", "nope")), (("z", "status"), ("history", "status")),
                             ("w_pen_l", ("history", "w_pen_l", "multipliers only")), (("cost", "w_pen_f"), ("history", "w_pen_f", "multipliers only"))):
            with pytest.raises(ilqg.IlqgError) as e:
                q.history(names)
            assert all(w in str(e.value) for w in words), str(e.value)
    assert lib.calls == []
    off = Recorder(cap=0)
    for q in (solver(ilqg, off), solver(ilqg, off, ilqg.MultiSolver)):
        with pytest.raises(ilqg.IlqgError) as e:
            q.history()
        assert "no iteration history" in str(e.value) and "set_history" in str(e.value)
    assert off.calls == []
    with_mul = solver(ilqg, Recorder((6, 6)))
    assert list(with_mul.history("w_pen_l")) == ["w_pen_l"]


def test_methods_of_an_old_library_say_rebuild(ilqg):
    s, m = solver(ilqg, OldLibrary()), solver(ilqg, OldLibrary(), ilqg.MultiSolver)
    for call, name in ((lambda: s.set_history(4), BATCH[0]), (lambda: s.set_history(0), BATCH[0]), (lambda: s.history(), BATCH[1]),
                       (lambda: m.set_history(4), MULTI[0]), (lambda: m.history("n"), MULTI[1])):
        with pytest.raises(ilqg.IlqgError) as e:
            call()
        assert name in str(e.value) and "rebuild" in str(e.value)


def test_public_header_declares_the_entries_and_states_the_rule():
    text = open(os.path.join(ROOT, "include", "ilqg_batch.h")).read()
    for entry in BATCH + MULTI:
        assert re.search(r"\bint %s\(" % entry, text), entry
    flat = " ".join(re.sub(r"\n \*", "\n", text).split()).lower()  # (comment lines joined)
    for words in ("it first appends one entry for every trajectory that is active",                     # append before the update
                  "exactly those whose line search has just run",
                  "appends nothing, as the reference writes no log for it",
                  "ilqg_batch_set_history and ilqg_batch_init clear counts and entries",
                  "ilqg_batch_shift and the resident loops do not",
                  "entries at positions >= cap are dropped while n counts on",
                  "unwritten entries read as zero",
                  "n_alpha + 1 = none accepted",
                  "before the update moves it",
                  "ilqg_batch_solve_stream refuses a batch with a history",
                  "it belongs to slots, starts pass through them",
                  "ilqg_batch_set_history(c, 0)"):
        assert words in flat, words
    for refusal in ("cap < 0", "a capacity the device has no memory for", "a getter without a history", "an unknown name",
                    "w_pen_* without multipliers", "out = null"):
        assert refusal in flat, refusal
    for name in DOUBLES + PENALTIES + INTS:
        assert re.search(r"\b%s\b" % re.escape(name.lower()), flat), name
    ilqg = load_package().ilqg
    doc = " ".join(ilqg.BatchSolver.set_history.__doc__.split())
    assert "first appends one entry for every trajectory that is active" in doc and "dropped while n counts on" in doc
    assert "init() clear" in doc and "shift() and the resident loops do not" in doc and "solve_stream refuses" in doc


def test_the_shim_and_the_host_name_the_same_fields():
    """the one table of names (ilqg_host.c history_names[]) covers every field of the shim's two enums and nothing else, the timing
    slot is the last of ILQG_K_*, and history_cases.DEFAULT_ALPHA is the step-size list of standard_parameters()"""
    csrc = os.path.join(ROOT, "ddp-generator_amd", "csrc")
    shim, host, impl = (open(os.path.join(csrc, f)).read() for f in ("ilqg_shim.h", "ilqg_host.c", "ilqg_shim_impl.inc"))
    table = re.search(r"history_names\[\] = \{(.*?)\n\};", host, re.S).group(1)
    rows = re.findall(r'\{"(\w+)", (\d), (ILQG_HI?_\w+)\}', table)
    assert [r[0] for r in rows] == list(DOUBLES + PENALTIES + INTS + ("n",))
    assert all((r[1] == "1") == r[2].startswith("ILQG_HI_") for r in rows)
    fields = re.findall(r"\b(ILQG_HI?_[A-Z0-9_]+)\b", shim)
    assert {f for f in fields if not f.endswith("_COUNT")} == {r[2] for r in rows}
    kernels = re.search(r"enum \{\s*ILQG_K_DERIVS = 0,(.*?)ILQG_K_COUNT", shim, re.S).group(1)
    assert re.findall(r"ILQG_K_\w+", kernels)[-1] == "ILQG_K_HISTORY"
    assert re.search(r'"k_shift_windows", "k_history"\};', impl)
    alpha = re.search(r"ilqg_default_alpha\[8\] = \{(.*?)\};", host, re.S).group(1)
    assert tuple(float(v) for v in alpha.replace("\n", " ").split(",")) == DEFAULT_ALPHA
