"""ilqg.py's side of BatchSolver.set_param_steps_batch / param_steps_batch / shift_param_batch and the two MultiSolver forms,
where no GPU is needed: the rows [B, n_hor+1] and the tails [B, steps] reach the entries as documented (single precision and
strided inputs copied) with the name; None clears the name (values NULL) or holds the last value (tail NULL); wrong shapes,
unknown and fixed-size names, host arrays with device=True (and the reverse) are refused before any library call; a library
built before the entries existed says "rebuild"; and the public header declares the seven entries and states the refusals.
Modelled on tests/test_params_batch_binding.py."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from conftest import ROOT, load_package
from test_policy_rollout_binding import FakeCudaTensor, OldLibrary
from test_policy_rollout_params_binding import B, N, solver

NEW = ["ilqg_batch_set_param_steps_batch", "ilqg_batch_set_param_steps_batch_device", "ilqg_batch_get_param_steps_batch",
       "ilqg_batch_shift_param_batch", "ilqg_batch_shift_param_batch_device", "ilqg_multi_set_param_steps_batch",
       "ilqg_multi_shift_param_batch"]


def doubles(ptr, shape):
    if ptr is None:
        return None
    return np.ctypeslib.as_array(C.cast(ptr, C.POINTER(C.c_double)), shape=(int(np.prod(shape)),)).reshape(shape).copy()


class Recorder:
    """a library with the new entries: remembers what each was called with, rows and tails as values"""

    def __init__(self):
        self.calls = []
        for name in (NEW[0], NEW[5]):
            setattr(self, name, self._set(name))
        for name in (NEW[3], NEW[6]):
            setattr(self, name, self._shift(name))
        setattr(self, NEW[2], self._get)

    def _set(self, entry):
        def call(h, name, values):
            self.calls.append((entry, dict(h=h, name=name.decode(), rows=doubles(values, (B, N + 1)))))
            return 0
        return call

    def _shift(self, entry):
        def call(h, name, steps, tail):
            self.calls.append((entry, dict(h=h, name=name.decode(), steps=steps, tail=doubles(tail, (B, max(steps, 0))))))
            return 0
        return call

    def _get(self, h, name, out):
        a = np.ctypeslib.as_array(C.cast(out, C.POINTER(C.c_double)), shape=(B * (N + 1),))
        a[:] = np.arange(B * (N + 1))
        self.calls.append((NEW[2], dict(h=h, name=name.decode())))
        return 0


@pytest.fixture(scope="module")
def ilqg():
    return load_package().ilqg


def test_rows_and_tails_reach_the_entries_as_documented(ilqg):
    lib = Recorder()
    s, m = solver(ilqg, lib), solver(ilqg, lib, ilqg.MultiSolver)
    rng = np.random.default_rng(1)
    rows, tail = rng.standard_normal((B, N + 1)), rng.standard_normal((B, 3))
    s.set_param_steps_batch("vref", rows)
    s.set_param_steps_batch("vref", rows.astype(np.float32))                  # single precision: converted
    s.set_param_steps_batch("vref", np.zeros((B, 2 * (N + 1)))[:, ::2] + rows)  # strided: copied
    s.set_param_steps_batch("vref", rows.tolist())
    m.set_param_steps_batch("vref", rows)
    s.shift_param_batch("vref", 3, tail)
    s.shift_param_batch("vref", 3, np.asfortranarray(tail))
    m.shift_param_batch("vref", 3, tail)
    calls = lib.calls
    assert [c[0] for c in calls] == [NEW[0]] * 4 + [NEW[5]] + [NEW[3]] * 2 + [NEW[6]]
    for (name, c), w in zip(calls[:5], [rows, rows.astype(np.float32).astype(np.float64), rows, rows, rows]):
        assert c["h"] == 1 and c["name"] == "vref" and np.array_equal(c["rows"], w), name
    for name, c in calls[5:]:
        assert c["h"] == 1 and c["name"] == "vref" and c["steps"] == 3 and np.array_equal(c["tail"], tail), name


def test_none_clears_the_name_and_holds_the_last_value(ilqg):
    lib = Recorder()
    s, m = solver(ilqg, lib), solver(ilqg, lib, ilqg.MultiSolver)
    for q in (s, m):
        q.set_param_steps_batch("vref", None)
        q.shift_param_batch("vref", 4)
    s.set_param_steps_batch("vref", None, device=True)  # (nothing to read: the host entry)
    s.shift_param_batch("vref", 4, None, device=True)
    assert [c[0] for c in lib.calls] == [NEW[0], NEW[3], NEW[5], NEW[6], NEW[0], NEW[3]]
    for _, c in lib.calls:
        assert c.get("rows", None) is None and c.get("tail", None) is None and c["name"] == "vref"


def test_the_getter_returns_a_row_per_trajectory(ilqg):
    lib = Recorder()
    s = solver(ilqg, lib)
    out = s.param_steps_batch("vref")
    assert out.shape == (B, N + 1) and np.array_equal(out.reshape(-1), np.arange(B * (N + 1)))
    assert lib.calls == [(NEW[2], dict(h=1, name="vref"))]


def test_wrong_arguments_are_refused_before_any_library_call(ilqg):
    lib = Recorder()
    s, m = solver(ilqg, lib), solver(ilqg, lib, ilqg.MultiSolver)
    good = np.zeros((B, N + 1))
    for q in (s, m):
        for call, words in ((lambda: q.set_param_steps_batch("nope", good), ("name", "Parameter name 'nope' is not member of parameters struct.")),
                            (lambda: q.set_param_steps_batch("cf", good), ("name", "cf", "fixed size of 4", "set_params_batch")),
                            (lambda: q.set_param_steps_batch("nope", None), ("nope", "not member")),
                            (lambda: q.set_param_steps_batch("vref", np.zeros((B, N))), ("values", "shape", "(5, 13)")),
                            (lambda: q.set_param_steps_batch("vref", np.zeros((N + 1, B))), ("values", "shape")),
                            (lambda: q.set_param_steps_batch("vref", np.zeros(N + 1)), ("values", "shape")),     # a shared window is no table
                            (lambda: q.set_param_steps_batch("vref", FakeCudaTensor((B, N + 1))), ("values", "device=True")),
                            (lambda: q.shift_param_batch("nope", 1), ("nope", "not member")),
                            (lambda: q.shift_param_batch("d", 1), ("d", "fixed size of 1")),
                            (lambda: q.shift_param_batch("vref", 3, np.zeros((B, 2))), ("tail", "shape", "(5, 3)")),
                            (lambda: q.shift_param_batch("vref", 3, np.zeros(3)), ("tail", "shape")),             # a shared tail is no table
                            (lambda: q.shift_param_batch("vref", 3, FakeCudaTensor((B, 3))), ("tail", "device=True"))):
            with pytest.raises(ilqg.IlqgError) as e:
                call()
            assert all(w in str(e.value) for w in words), str(e.value)
    with pytest.raises(ilqg.IlqgError) as e:
        s.param_steps_batch("cf")
    assert "fixed size" in str(e.value)
    assert lib.calls == []


def test_device_arguments_are_checked_before_any_library_call(ilqg):
    import torch
    lib = Recorder()
    setattr(lib, NEW[1], None)
    setattr(lib, NEW[4], None)
    s = solver(ilqg, lib)
    for a, words in ((np.zeros((B, N + 1)), ("host",)), (torch.zeros((B, N + 1), dtype=torch.float64), ("host",)),
                     (FakeCudaTensor((B, N + 1), dtype="torch.float32"), ("float64",)), (FakeCudaTensor((B, N + 1), contiguous=False), ("contiguous",)),
                     (FakeCudaTensor((B, N + 1), index=1), ("GPU",)), (FakeCudaTensor((B, N)), ("shape", "(5, 13)"))):
        with pytest.raises(ilqg.IlqgError) as e:
            s.set_param_steps_batch("vref", a, device=True)
        assert "values" in str(e.value) and all(w in str(e.value) for w in words), str(e.value)
    for a, words in ((np.zeros((B, 3)), ("host",)), (FakeCudaTensor((B, 3), dtype="torch.float32"), ("float64",)),
                     (FakeCudaTensor((B, 3), contiguous=False), ("contiguous",)), (FakeCudaTensor((B, 3), index=1), ("GPU",)),
                     (FakeCudaTensor((B, 2)), ("shape", "(5, 3)"))):
        with pytest.raises(ilqg.IlqgError) as e:
            s.shift_param_batch("vref", 3, a, device=True)
        assert "tail" in str(e.value) and all(w in str(e.value) for w in words), str(e.value)
    assert lib.calls == []


def test_methods_of_an_old_library_say_rebuild(ilqg):
    rows, tail = np.zeros((B, N + 1)), np.zeros((B, 2))
    s, m = solver(ilqg, OldLibrary()), solver(ilqg, OldLibrary(), ilqg.MultiSolver)
    for call, name in ((lambda: s.set_param_steps_batch("vref", rows), NEW[0]), (lambda: s.set_param_steps_batch("vref", None), NEW[0]),
                       (lambda: s.set_param_steps_batch("vref", FakeCudaTensor((B, N + 1)), device=True), NEW[1]),
                       (lambda: s.param_steps_batch("vref"), NEW[2]), (lambda: s.shift_param_batch("vref", 2, tail), NEW[3]),
                       (lambda: s.shift_param_batch("vref", 2), NEW[3]),
                       (lambda: s.shift_param_batch("vref", 2, FakeCudaTensor((B, 2)), device=True), NEW[4]),
                       (lambda: m.set_param_steps_batch("vref", rows), NEW[5]), (lambda: m.shift_param_batch("vref", 2, tail), NEW[6])):
        with pytest.raises(ilqg.IlqgError) as e:
            call()
        assert name in str(e.value) and "rebuild" in str(e.value)


def test_public_header_declares_the_entries_and_states_the_refusals():
    text = open(os.path.join(ROOT, "include", "ilqg_batch.h")).read()
    for entry in NEW:
        assert re.search(r"\bint %s\(" % entry, text), entry
    flat = " ".join(re.sub(r"\n \*", "\n", text).split()).lower()  # (comment lines joined)
    assert "values = null makes that name shared again" in flat
    assert "bit for bit what re-sending [rows[:, steps:], tail] through the setter gives" in flat
    assert "the rows travel with their trajectories" in flat
    for refusal in ("a fixed-size name", "steps out of range", "ilqg_batch_shift_param_batch of a name that is currently shared",
                    "not device memory of the context's device", "ilqg_batch_set_param and ilqg_batch_shift_param of a name that currently is per-trajectory",
                    "ilqg_batch_solve_stream while any name has rows", "wave mapping"):
        assert refusal in flat, refusal
    for out_of_scope in ("the wave, row and quad mappings", "the drop-in ilqg()", "rows per start in ilqg_batch_solve_stream",
                         "receding / receding_plant for problems with per-time-step parameters"):
        assert out_of_scope in flat, out_of_scope
