"""ilqg.py's side of BatchSolver.receding_plant / MultiSolver.receding_plant, where no GPU is needed: the arguments reach
ilqg_batch_receding_plant / ilqg_multi_receding_plant as documented (the parameter rows packed [B, W] in dict order with the
matching names, the size-1 axis left out, single precision and strided inputs copied, None as NULL and n_names = 0, x_plant
copied so that the caller's array is not written); wrong shapes and dtypes, device tensors, unknown and per-time-step names
and an empty dict are refused before any library call; a library built before the entries existed says "rebuild"; the
C entry of several shards offsets every array by the shard's first trajectory; and the public header declares the two
entries and states the semantics."""
import ctypes as C
import os
import re
import types

import numpy as np
import pytest

from conftest import ROOT, load_package
from test_policy_rollout_binding import FakeCudaTensor, OldLibrary

NEW = ["ilqg_batch_receding_plant", "ilqg_multi_receding_plant"]
B, N, NX, NU = 5, 12, 4, 2
PARAMS = [("h", 1), ("cf", 4), ("vref", -1), ("limA", 2), ("d", 1)]  # paramdesc[] of the stand-in problem


def _doubles(p, shape):
    return None if p is None else np.ctypeslib.as_array(C.cast(p, C.POINTER(C.c_double)), shape=(int(np.prod(shape)),)).reshape(shape).copy()


class Recorder:
    """a library with the two entries: remembers what each was called with, the arrays as values, and fills the outputs"""

    def __init__(self):
        self.calls = []
        for name in NEW:
            setattr(self, name, self._entry(name))

    def _entry(self, name):
        def call(h, rounds, steps, iterations, feedback, x_plant, n_names, names, values, disturbance, x, u, cost, plan_cost, ok):
            got = [names[i].decode() for i in range(n_names)]
            W = sum(dict(PARAMS)[n] for n in got)
            self.calls.append((name, dict(h=h, rounds=rounds, steps=steps, iterations=iterations, feedback=feedback, names=got, names_arg=names,
                                          x_plant=_doubles(x_plant, (B, NX)), values=_doubles(values, (B, W)) if n_names else values,
                                          disturbance=_doubles(disturbance, (B, rounds * steps, NX)), out=(x, u, cost, plan_cost, ok))))
            if x_plant is not None:  # the final states
                np.ctypeslib.as_array(C.cast(x_plant, C.POINTER(C.c_double)), shape=(B * NX,))[:] = 9.0
            np.ctypeslib.as_array(C.cast(ok, C.POINTER(C.c_int)), shape=(B,))[:] = 1
            return 0
        return call


def solver(ilqg, lib, cls=None):
    s = object.__new__(cls or ilqg.BatchSolver)
    s.lib, s.h, s.B, s.N, s.device = lib, 1, B, N, 0
    s.problem = types.SimpleNamespace(nx=NX, nu=NU, params=list(PARAMS))
    return s


@pytest.fixture(scope="module")
def ilqg():
    return load_package().ilqg


def test_arguments_reach_the_entry_as_documented(ilqg):
    lib = Recorder()
    s, m = solver(ilqg, lib), solver(ilqg, lib, ilqg.MultiSolver)
    rng = np.random.default_rng(1)
    limA, d, cf = rng.standard_normal((B, 2)), rng.standard_normal((B, 1)), rng.standard_normal((B, 4))
    xp, w = rng.standard_normal((B, NX)), rng.standard_normal((B, 6, NX))
    keep = xp.copy()
    outs = [s.receding_plant(3, 2, 4, x_plant=xp, params=dict(limA=limA, d=d, cf=cf), disturbance=w),     # dict order, not paramdesc[] order
            s.receding_plant(3, 2, 4, feedback=False, params=dict(cf=cf, d=d[:, 0])),                      # the size-1 axis left out
            s.receding_plant(1, 6, 0, params=dict(cf=cf.astype(np.float32)), disturbance=np.zeros((B, 6, 2 * NX))[:, :, ::2] + w),  # converted, copied
            s.receding_plant(3, 2, 4),                                                                     # the plant is the model
            m.receding_plant(3, 2, 4, x_plant=xp, params=dict(d=d, limA=limA), disturbance=w)]
    calls = lib.calls
    assert [c[0] for c in calls] == [NEW[0]] * 4 + [NEW[1]]
    assert [c["names"] for _, c in calls] == [["limA", "d", "cf"], ["cf", "d"], ["cf"], [], ["d", "limA"]]
    assert [(c["rounds"], c["steps"], c["iterations"], c["feedback"]) for _, c in calls] == [(3, 2, 4, 1), (3, 2, 4, 0), (1, 6, 0, 1), (3, 2, 4, 1), (3, 2, 4, 1)]
    want = [np.concatenate([limA, d, cf], axis=-1), np.concatenate([cf, d], axis=-1), cf.astype(np.float32).astype(np.float64), None,
            np.concatenate([d, limA], axis=-1)]
    for (name, c), v in zip(calls, want):
        assert c["h"] == 1 and (c["values"] is None if v is None else np.array_equal(c["values"], v)), name
    assert calls[3][1]["names_arg"] is None and calls[3][1]["x_plant"] is None and calls[3][1]["disturbance"] is None
    for i in (0, 2, 4):
        assert np.array_equal(calls[i][1]["disturbance"], w)
    assert np.array_equal(calls[0][1]["x_plant"], keep) and np.array_equal(calls[4][1]["x_plant"], keep)
    assert np.array_equal(xp, keep), "the caller's x_plant was written"
    for out, given in zip(outs, (True, False, False, False, True)):
        assert sorted(out) == ["cost", "ok", "plan_cost", "u", "x", "x_plant"]
        r, n = (1, 6) if out is outs[2] else (3, 6)
        assert out["x"].shape == (B, n, NX) and out["u"].shape == (B, n, NU) and out["cost"].shape == (B, r) and out["plan_cost"].shape == (B, r)
        assert out["ok"].shape == (B,) and out["ok"].dtype == np.int32 and np.all(out["ok"] == 1)
        assert all(out[k].dtype == np.float64 and out[k].flags["C_CONTIGUOUS"] for k in ("x", "u", "cost", "plan_cost"))
        assert (np.all(out["x_plant"] == 9.0) and out["x_plant"].shape == (B, NX)) if given else out["x_plant"] is None
    assert all(p is not None for p in calls[0][1]["out"])


def test_wrong_arguments_are_refused_before_any_library_call(ilqg):
    lib = Recorder()
    s, m = solver(ilqg, lib), solver(ilqg, lib, ilqg.MultiSolver)
    good = dict(rounds=3, steps=2, iterations=4)
    bad = [(dict(x_plant=np.zeros((B, NX + 1))), ("x_plant", "shape", "(5, 4)")),
           (dict(x_plant=np.zeros((B - 1, NX))), ("x_plant", "shape")),
           (dict(x_plant=np.zeros((B, NX), dtype=complex)), ("x_plant", "dtype", "complex")),
           (dict(x_plant=FakeCudaTensor((B, NX))), ("x_plant", "device", "host memory")),
           (dict(disturbance=np.zeros((B, 5, NX))), ("disturbance", "shape", "(5, 6, 4)")),
           (dict(disturbance=np.zeros((B, 6, NX), dtype=object)), ("disturbance", "dtype")),
           (dict(disturbance=FakeCudaTensor((B, 6, NX))), ("disturbance", "device")),
           (dict(params=dict()), ("params", "non-empty")),
           (dict(params=[("d", np.zeros((B, 1)))]), ("params", "dict")),
           (dict(params=dict(cf=np.zeros((B, 3)))), ("params['cf']", "shape", "(5, 4)")),
           (dict(params=dict(cf=np.zeros(B))), ("params['cf']", "shape")),                 # the last axis only for size 1
           (dict(params=dict(cf=np.zeros((B, 3, 4)))), ("params['cf']", "shape")),         # no axis of roll-outs here
           (dict(params=dict(d=np.zeros((B + 1, 1)))), ("params['d']", "shape")),
           (dict(params=dict(d=np.array(["a"] * B))), ("params['d']", "dtype")),
           (dict(params=dict(nope=np.zeros((B, 1)))), ("params", "Parameter name 'nope' is not member of parameters struct.")),
           (dict(params=dict(vref=np.zeros((B, N + 1)))), ("params", "vref", "per-time-step parameters stay shared")),
           (dict(params=dict(d=FakeCudaTensor((B, 1)))), ("params['d']", "device")),
           (dict(rounds=3.5), ("rounds", "integer")),
           (dict(steps="2"), ("steps", "integer")),
           (dict(iterations=None), ("iterations", "integer"))]
    for change, words in bad:
        for q in (s, m):
            with pytest.raises(ilqg.IlqgError) as e:
                q.receding_plant(**dict(good, **change))
            assert "receding_plant" in str(e.value) and all(w in str(e.value) for w in words), str(e.value)
    assert lib.calls == []


def test_methods_of_an_old_library_say_rebuild(ilqg):
    s, m = solver(ilqg, OldLibrary()), solver(ilqg, OldLibrary(), ilqg.MultiSolver)
    for call, name in ((lambda: s.receding_plant(3, 2, 4), NEW[0]), (lambda: m.receding_plant(3, 2, 4, params=dict(d=np.zeros(B))), NEW[1])):
        with pytest.raises(ilqg.IlqgError) as e:
            call()
        assert name in str(e.value) and "rebuild" in str(e.value)


def test_the_multi_entry_offsets_every_array_by_the_shards_first_trajectory():
    """read off the C source: the host code cannot run without a GPU, and the shards' offsets are one expression each"""
    text = open(os.path.join(ROOT, "ddp-generator_amd", "csrc", "ilqg_host.c")).read()
    body = text[text.index("static int multi_receding_plant("):]  # the one worker of both multi entries
    body = " ".join(body[body.index("{"):body.index("\n}\n")].split())
    entry = text[text.index("\nint ilqg_multi_receding_plant("):]
    entry = " ".join(entry[entry.index("{") + 1:entry.index("\n}\n")].split())
    assert "at = (size_t)m->first[g]" in body and "per = rn * (steps > 0 ? (size_t)steps : 0)" in body
    for piece in ("x_plant ? x_plant + at * N_X : NULL", "values ? values + at * W : NULL", "disturbance ? disturbance + at * per * N_X : NULL",
                  "x_applied ? x_applied + at * per * N_X : NULL", "u_applied ? u_applied + at * per * N_U : NULL",
                  "cost_applied ? cost_applied + at * rn : NULL", "plan_cost ? plan_cost + at * rn : NULL", "ok ? ok + at : NULL"):
        assert body.count(piece) == 1, piece
    # the entry reaches the shard's ilqg_batch_receding_plant through the worker: its not-windowed branch, fed the offset pointers
    assert entry.startswith("return multi_receding_plant(m, 0, rounds, steps, iterations, feedback, x_plant, n_names, names, values, disturbance, 0, NULL, NULL,")
    assert ": ilqg_batch_receding_plant(m->shard[g], rounds, steps, iterations, feedback, xp, n_names, names, v, w, xa, ua, ca, pc, okg)" in body


def test_public_header_declares_the_entries_and_states_the_semantics():
    text = open(os.path.join(ROOT, "include", "ilqg_batch.h")).read()
    for entry in NEW:
        assert re.search(r"\bint %s\(" % entry, text), entry
    flat = " ".join(re.sub(r"\n \*", "\n", text).split()).lower()  # (comment lines joined)
    for words in ("advances `steps` steps from its own state", "evaluated under the plant's parameters", "ilqg_batch_shift(c, steps, x0_new = xp, u_tail = null)",
                  "failure is per trajectory", "it stays at its last finite state", "all outputs null is not a no-op",
                  "between rounds the host waits for nothing and copies nothing", "n_names = 0 (names and values are then not read): the plant is the model"):
        assert words in flat, words
    ilqg = load_package().ilqg
    doc = " ".join(ilqg.BatchSolver.receding_plant.__doc__.split())
    assert "x_plant" in doc and "disturbance" in doc and "the planner keeps the batch's parameters" in doc
