"""ilqg.py's side of policy_rollout(params=...), where no GPU is needed: the packed values reach
ilqg_batch_policy_rollout_params / ilqg_multi_policy_rollout_params as documented (dict order, [B, R, W] and [R, W], the
size-1 axis left out, single precision and strided inputs copied, `shared` only for the [R, ...] form) with the matching
array of names; params=None calls the OLD entry with the old argument list; wrong shapes, mixed forms, an R that differs
from the starts', an empty dict and host arrays with device=True (and the reverse) are refused before any library call; a
library built before the entries existed says "rebuild"; and the public header declares the three entries and states the
semantics."""
import ctypes as C
import os
import re
import types

import numpy as np
import pytest

from conftest import ROOT, load_package
from test_policy_rollout_binding import FakeCudaTensor, OldLibrary
from test_policy_rollout_binding import Recorder as OldEntries

NEW = ["ilqg_batch_policy_rollout_params", "ilqg_batch_policy_rollout_params_device", "ilqg_multi_policy_rollout_params"]
B, N, NX, NU = 5, 12, 4, 2
PARAMS = [("h", 1), ("cf", 4), ("vref", -1), ("limA", 2), ("d", 1)]  # paramdesc[] of the stand-in problem


class Recorder(OldEntries):
    """a library with the old and the new entries: remembers what each was called with, names and values as values"""

    def __init__(self):
        OldEntries.__init__(self)
        for name in NEW:
            setattr(self, name, self._params_entry(name))

    def _params_entry(self, name):
        def call(h, R, x0, n_names, names, values, shared, alpha, feedback, cost, ok, x_end, x, u, *stream):
            got = [names[i].decode() for i in range(n_names)]
            W = sum(dict(PARAMS)[n] for n in got)
            table = None
            if name != NEW[1]:
                rows = (R,) if shared else (B, R)
                table = np.ctypeslib.as_array(C.cast(values, C.POINTER(C.c_double)), shape=(int(np.prod(rows)) * W,)).reshape(rows + (W,)).copy()
            self.calls.append((name, dict(h=h, R=R, names=got, table=table, values=values, shared=shared, alpha=alpha, feedback=feedback,
                                          out=(cost, ok, x_end, x, u), stream=stream)))
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


def test_packed_values_and_names_reach_the_entry_as_documented(ilqg):
    lib = Recorder()
    s, m = solver(ilqg, lib), solver(ilqg, lib, ilqg.MultiSolver)
    x0 = np.zeros((B, 3, NX))
    rng = np.random.default_rng(1)
    limA, d, cf = rng.standard_normal((B, 3, 2)), rng.standard_normal((B, 3, 1)), rng.standard_normal((B, 3, 4))
    s.policy_rollout(x0, params=dict(limA=limA, d=d, cf=cf))                      # dict order, not paramdesc[] order
    s.policy_rollout(x0, params=dict(cf=cf, d=d[:, :, 0]))                        # the size-1 axis left out
    s.policy_rollout(x0, alpha=0.25, feedback=False, params=dict(d=d[0, :, 0], limA=limA[0]))  # [R] and [R, size]: one table for all
    s.policy_rollout(x0, params=dict(cf=cf.astype(np.float32)))                    # single precision: converted
    s.policy_rollout(x0, params=dict(limA=np.zeros((B, 3, 4))[:, :, ::2] + limA))  # strided: copied
    m.policy_rollout(x0, trajectories=True, params=dict(d=d, limA=limA))
    m.policy_rollout(x0[0], params=dict(h=d[0]))
    calls = lib.calls
    assert [c[0] for c in calls] == [NEW[0]] * 5 + [NEW[2]] * 2
    assert [c["names"] for _, c in calls] == [["limA", "d", "cf"], ["cf", "d"], ["d", "limA"], ["cf"], ["limA"], ["d", "limA"], ["h"]]
    assert [c["shared"] for _, c in calls] == [0, 0, 1, 0, 0, 0, 1]
    want = [np.concatenate([limA, d, cf], axis=-1), np.concatenate([cf, d], axis=-1), np.concatenate([d[0], limA[0]], axis=-1),
            cf.astype(np.float32).astype(np.float64), limA, np.concatenate([d, limA], axis=-1), d[0]]
    for (name, c), w in zip(calls, want):
        assert c["h"] == 1 and c["R"] == 3 and c["table"].shape == w.shape and np.array_equal(c["table"], w), name
    assert [(c["alpha"], c["feedback"]) for _, c in calls[:3]] == [(1.0, 1), (1.0, 1), (0.25, 0)]
    cost, ok, x_end, x, u = calls[0][1]["out"]
    assert cost and ok and x_end and x is None and u is None
    assert all(p is not None for p in calls[5][1]["out"])


def test_without_params_the_old_entry_gets_the_old_arguments(ilqg):
    lib = Recorder()
    s, m = solver(ilqg, lib), solver(ilqg, lib, ilqg.MultiSolver)
    x0 = np.arange(B * 3 * NX, dtype=np.float64).reshape(B, 3, NX)
    s.policy_rollout(x0, alpha=0.5, params=None)
    m.policy_rollout(x0)
    assert [c[0] for c in lib.calls] == ["ilqg_batch_policy_rollout", "ilqg_multi_policy_rollout"]
    for _, c in lib.calls:  # (the old recorder's entry takes exactly the old argument list)
        assert c["R"] == 3 and np.array_equal(c["starts"], x0) and c["stream"] == ()
    assert lib.calls[0][1]["alpha"] == 0.5


def test_wrong_params_are_refused_before_any_library_call(ilqg):
    lib = Recorder()
    s, m = solver(ilqg, lib), solver(ilqg, lib, ilqg.MultiSolver)
    x0 = np.zeros((B, 3, NX))
    bad = [(dict(), ("params", "non-empty")),
           ([("d", np.zeros((B, 3)))], ("params", "dict")),
           (dict(cf=np.zeros((B, 3, 3))), ("params", "cf", "shape", "(5, 3, 4)")),
           (dict(cf=np.zeros((B, 3))), ("params", "cf", "shape")),                      # the last axis only for size 1
           (dict(cf=np.zeros((B, 4, 4))), ("params", "cf", "(5, 3, 4)", "R = 3")),    # R differs from the starts'
           (dict(d=np.zeros((4,))), ("params", "d", "(3, 1)")),
           (dict(cf=np.zeros((B + 1, 3, 4))), ("params", "cf", "shape")),
           (dict(cf=np.zeros((B, 3, 4)), d=np.zeros(3)), ("params", "mixes", "cf", "d")),  # mixed forms
           (dict(nope=np.zeros((B, 3, 1))), ("params", "Parameter name 'nope' is not member of parameters struct.")),
           (dict(vref=np.zeros((B, 3, N + 1))), ("params", "vref", "per-time-step parameters stay shared")),
           (dict(d=FakeCudaTensor((B, 3, 1))), ("params", "d", "device=True"))]
    for params, words in bad:
        for q in (s, m):
            with pytest.raises(ilqg.IlqgError) as e:
                q.policy_rollout(x0, params=params)
            assert all(w in str(e.value) for w in words), str(e.value)
    assert lib.calls == []


def test_device_params_are_checked_before_any_library_call(ilqg):
    import torch
    lib = Recorder()
    s = solver(ilqg, lib)
    x0 = FakeCudaTensor((B, 3, NX))
    good = FakeCudaTensor((B, 3, 4))
    for params, words in ((dict(cf=np.zeros((B, 3, 4))), ("params", "cf", "host")),
                          (dict(cf=torch.zeros((B, 3, 4), dtype=torch.float64)), ("params", "cf", "host")),
                          (dict(cf=good, d=np.zeros((B, 3))), ("params", "'d'", "host")),
                          (dict(cf=FakeCudaTensor((B, 3, 4), dtype="torch.float32")), ("params", "cf", "float64")),
                          (dict(cf=FakeCudaTensor((B, 3, 4), contiguous=False)), ("params", "cf", "contiguous")),
                          (dict(cf=FakeCudaTensor((B, 3, 4), index=1)), ("params", "cf", "GPU")),
                          (dict(cf=FakeCudaTensor((B, 2, 4))), ("params", "cf", "shape", "R = 3")),
                          (dict(cf=good, d=FakeCudaTensor((3,))), ("params", "mixes")),
                          (dict(), ("params", "non-empty")),
                          (dict(vref=FakeCudaTensor((B, 3, N + 1))), ("params", "vref", "stay shared"))):
        with pytest.raises(ilqg.IlqgError) as e:
            s.policy_rollout(x0, device=True, params=params)
        assert all(w in str(e.value) for w in words), str(e.value)
    with pytest.raises(ilqg.IlqgError) as e:  # host starts with device tensors
        s.policy_rollout(np.zeros((B, 3, NX)), device=True, params=dict(cf=good))
    assert "x0" in str(e.value) and "host" in str(e.value)
    assert lib.calls == []


def test_methods_of_an_old_library_say_rebuild(ilqg):
    x0 = np.zeros((B, 3, NX))
    p = dict(d=np.zeros((B, 3)))
    for lib in (OldLibrary(), OldEntries()):  # without any roll-out entry, and with the plain ones only
        s, m = solver(ilqg, lib), solver(ilqg, lib, ilqg.MultiSolver)
        for call, name in ((lambda: s.policy_rollout(x0, params=p), NEW[0]),
                           (lambda: s.policy_rollout(FakeCudaTensor((B, 3, NX)), device=True, params=dict(d=FakeCudaTensor((B, 3)))), NEW[1]),
                           (lambda: m.policy_rollout(x0, params=p), NEW[2])):
            with pytest.raises(ilqg.IlqgError) as e:
                call()
            assert name in str(e.value) and "rebuild" in str(e.value)


def test_public_header_declares_the_entries_and_states_the_semantics():
    text = open(os.path.join(ROOT, "include", "ilqg_batch.h")).read()
    for entry in NEW:
        assert re.search(r"\bint %s\(" % entry, text), entry
    flat = " ".join(re.sub(r"\n \*", "\n", text).split()).lower()  # (comment lines joined)
    assert "named parameters replace the batch's" in flat
    assert "per-time-step parameters (size -1) stay shared" in flat
    assert "the gains having been computed under the batch's parameters" in flat
    assert "is not member of parameters struct." in flat
    ilqg = load_package().ilqg
    assert "params" in ilqg.BatchSolver.policy_rollout.__doc__ and "gains were computed under the batch's parameters" in " ".join(ilqg.BatchSolver.policy_rollout.__doc__.split())
