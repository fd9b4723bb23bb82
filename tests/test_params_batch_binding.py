"""ilqg.py's side of BatchSolver.set_params_batch / params_batch / MultiSolver.set_params_batch, where no GPU is needed: the
packed rows reach ilqg_batch_set_params_batch / ilqg_multi_set_params_batch as documented (dict order, [B, W], the size-1 axis
left out, single precision and strided inputs copied) with the matching array of names; {} and None clear the set (n_names =
0, no names, no values); wrong shapes, unknown and per-time-step names, host arrays with device=True (and the reverse) are
refused before any library call; a library built before the entries existed says "rebuild"; and the public header declares the
four entries and states the order rule and the refusals.  Modelled on tests/test_policy_rollout_params_binding.py."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from conftest import ROOT, load_package
from test_policy_rollout_binding import FakeCudaTensor, OldLibrary
from test_policy_rollout_params_binding import PARAMS, B, N, Recorder as OldEntries, solver

NEW = ["ilqg_batch_set_params_batch", "ilqg_batch_set_params_batch_device", "ilqg_batch_get_params_batch", "ilqg_multi_set_params_batch"]


class Recorder(OldEntries):
    """a library with the roll-out entries and the new ones: remembers what each was called with, names and rows as values"""

    def __init__(self):
        OldEntries.__init__(self)
        for name in (NEW[0], NEW[3]):
            setattr(self, name, self._set_entry(name))
        setattr(self, NEW[1], self._set_entry(NEW[1]))
        setattr(self, NEW[2], self._get_entry)

    def _set_entry(self, name):
        def call(h, n_names, names, values, *stream):
            got = [names[i].decode() for i in range(n_names)]
            W = sum(dict(PARAMS)[n] for n in got)
            table = None
            if n_names and name != NEW[1]:
                table = np.ctypeslib.as_array(C.cast(values, C.POINTER(C.c_double)), shape=(B * W,)).reshape(B, W).copy()
            self.calls.append((name, dict(h=h, n_names=n_names, names=got, names_arg=names, table=table, values=values, stream=stream)))
            return 0
        return call

    def _get_entry(self, h, name, out):
        size = dict(PARAMS)[name.decode()]
        a = np.ctypeslib.as_array(C.cast(out, C.POINTER(C.c_double)), shape=(B * size,))
        a[:] = np.arange(B * size)
        self.calls.append((NEW[2], dict(h=h, name=name.decode())))
        return 0


@pytest.fixture(scope="module")
def ilqg():
    return load_package().ilqg


def test_packed_rows_and_names_reach_the_entry_as_documented(ilqg):
    lib = Recorder()
    s, m = solver(ilqg, lib), solver(ilqg, lib, ilqg.MultiSolver)
    rng = np.random.default_rng(1)
    limA, d, cf = rng.standard_normal((B, 2)), rng.standard_normal((B, 1)), rng.standard_normal((B, 4))
    s.set_params_batch(dict(limA=limA, d=d, cf=cf))                       # dict order, not paramdesc[] order
    s.set_params_batch(dict(cf=cf, d=d[:, 0]))                            # the [B] form of a size-1 parameter
    s.set_params_batch(dict(cf=cf.astype(np.float32)))                    # single precision: converted
    s.set_params_batch(dict(limA=np.zeros((B, 4))[:, ::2] + limA))        # strided: copied
    m.set_params_batch(dict(d=d, limA=limA))
    calls = lib.calls
    assert [c[0] for c in calls] == [NEW[0]] * 4 + [NEW[3]]
    assert [c["names"] for _, c in calls] == [["limA", "d", "cf"], ["cf", "d"], ["cf"], ["limA"], ["d", "limA"]]
    want = [np.concatenate([limA, d, cf], axis=-1), np.concatenate([cf, d], axis=-1), cf.astype(np.float32).astype(np.float64), limA,
            np.concatenate([d, limA], axis=-1)]
    for (name, c), w in zip(calls, want):
        assert c["h"] == 1 and c["stream"] == () and c["table"].shape == w.shape and np.array_equal(c["table"], w), name


def test_an_empty_dict_and_none_clear_the_set(ilqg):
    lib = Recorder()
    s, m = solver(ilqg, lib), solver(ilqg, lib, ilqg.MultiSolver)
    for q in (s, m):
        q.set_params_batch({})
        q.set_params_batch(None)
    s.set_params_batch({}, device=True)  # (nothing to read: the host entry)
    assert [c[0] for c in lib.calls] == [NEW[0]] * 2 + [NEW[3]] * 2 + [NEW[0]]
    for _, c in lib.calls:
        assert c["n_names"] == 0 and c["names_arg"] is None and c["values"] is None


def test_the_getter_returns_rows_of_the_parameters_size(ilqg):
    lib = Recorder()
    s = solver(ilqg, lib)
    for name, size in (("cf", 4), ("d", 1)):
        out = s.params_batch(name)
        assert out.shape == (B, size) and np.array_equal(out.reshape(-1), np.arange(B * size))
    assert [c[1]["name"] for c in lib.calls] == ["cf", "d"]


def test_wrong_params_are_refused_before_any_library_call(ilqg):
    lib = Recorder()
    s, m = solver(ilqg, lib), solver(ilqg, lib, ilqg.MultiSolver)
    bad = [([("d", np.zeros(B))], ("params", "dict")),
           (dict(cf=np.zeros((B, 3))), ("params", "cf", "shape", "(5, 4)")),
           (dict(cf=np.zeros(B)), ("params", "cf", "shape")),                  # the last axis only for size 1
           (dict(d=np.zeros((B, 2))), ("params", "d", "(5, 1)", "(5,)")),
           (dict(cf=np.zeros((B + 1, 4))), ("params", "cf", "shape")),
           (dict(cf=np.zeros((B, 3, 4))), ("params", "cf", "shape")),         # a roll-out table is not a trajectory table
           (dict(nope=np.zeros((B, 1))), ("params", "Parameter name 'nope' is not member of parameters struct.")),
           (dict(vref=np.zeros((B, N + 1))), ("params", "vref", "per-time-step parameters stay shared")),
           (dict(d=FakeCudaTensor((B, 1))), ("params", "d", "device=True"))]   # host / device mismatch
    for params, words in bad:
        for q in (s, m):
            with pytest.raises(ilqg.IlqgError) as e:
                q.set_params_batch(params)
            assert all(w in str(e.value) for w in words), str(e.value)
    assert lib.calls == []


def test_device_params_are_checked_before_any_library_call(ilqg):
    import torch
    lib = Recorder()
    s = solver(ilqg, lib)
    good = FakeCudaTensor((B, 4))
    for params, words in ((dict(cf=np.zeros((B, 4))), ("params", "cf", "host")),                        # host / device mismatch
                          (dict(cf=torch.zeros((B, 4), dtype=torch.float64)), ("params", "cf", "host")),
                          (dict(cf=good, d=np.zeros(B)), ("params", "'d'", "host")),
                          (dict(cf=FakeCudaTensor((B, 4), dtype="torch.float32")), ("params", "cf", "float64")),
                          (dict(cf=FakeCudaTensor((B, 4), contiguous=False)), ("params", "cf", "contiguous")),
                          (dict(cf=FakeCudaTensor((B, 4), index=1)), ("params", "cf", "GPU")),
                          (dict(cf=FakeCudaTensor((B, 3))), ("params", "cf", "shape", "(5, 4)")),
                          (dict(vref=FakeCudaTensor((B, N + 1))), ("params", "vref", "stay shared"))):
        with pytest.raises(ilqg.IlqgError) as e:
            s.set_params_batch(params, device=True)
        assert all(w in str(e.value) for w in words), str(e.value)
    assert lib.calls == []


def test_methods_of_an_old_library_say_rebuild(ilqg):
    p = dict(d=np.zeros(B))
    for lib in (OldLibrary(), OldEntries()):  # without any roll-out entry, and with those of the roll-outs only
        s, m = solver(ilqg, lib), solver(ilqg, lib, ilqg.MultiSolver)
        for call, name in ((lambda: s.set_params_batch(p), NEW[0]), (lambda: s.set_params_batch({}), NEW[0]),
                           (lambda: s.set_params_batch(dict(d=FakeCudaTensor((B,))), device=True), NEW[1]),
                           (lambda: s.params_batch("d"), NEW[2]), (lambda: m.set_params_batch(p), NEW[3]), (lambda: m.set_params_batch(None), NEW[3])):
            with pytest.raises(ilqg.IlqgError) as e:
                call()
            assert name in str(e.value) and "rebuild" in str(e.value)


def test_public_header_declares_the_entries_and_states_the_order_rule_and_the_refusals():
    text = open(os.path.join(ROOT, "include", "ilqg_batch.h")).read()
    for entry in NEW:
        assert re.search(r"\bint %s\(" % entry, text), entry
    flat = " ".join(re.sub(r"\n \*", "\n", text).split()).lower()  # (comment lines joined)
    assert "the trajectory's row first, then the roll-out's or the plant's row" in flat
    assert "per-time-step parameters (size -1) stay shared" in flat
    assert "replaces the whole per-trajectory set" in flat and "n_names = 0 clears it" in flat
    for refusal in ("a name given twice", "n_names < 0", "names or values null", "not device memory of the context's device",
                    "ilqg_batch_set_param of a name that currently is per-trajectory", "ilqg_batch_set_params_batch(c, 0, null, null)",
                    "wave mapping", "ilqg_batch_solve_stream is refused"):
        assert refusal in flat, refusal
    ilqg = load_package().ilqg
    doc = " ".join(ilqg.BatchSolver.set_params_batch.__doc__.split())
    assert "the trajectory's row first, then the roll-out's or the plant's" in doc and "{} or None clears it" in doc
