"""ilqg.py's side of BatchSolver.head / .shift (device tensors) / .shift_param and MultiSolver.head, where no GPU is needed:
a problem library built before the entries existed still loads and says "rebuild" when they are asked for; host arrays and
CPU tensors take the host entry in the documented shapes; a tensor on the device is checked BEFORE any library call; and
importing ilqg does not import torch."""
import ctypes as C
import os
import subprocess
import sys
import types

import numpy as np
import pytest

from conftest import ROOT, load_package

NEW = ["ilqg_batch_head", "ilqg_batch_head_device", "ilqg_batch_shift_device", "ilqg_batch_shift_param", "ilqg_multi_head"]
B, N, NX, NU = 5, 12, 4, 2


class OldLibrary:
    """stands for a CDLL without the new symbols"""


class Recorder:
    """stands for a library that has them: remembers what each entry was called with (`decode`, if set, turns the
    arguments into values while the caller's arrays are still alive)"""

    def __init__(self, decode=None):
        self.calls, self.decode = [], decode
        for name in NEW + ["ilqg_batch_shift"]:
            setattr(self, name, self._entry(name))

    def _entry(self, name):
        def call(*args):
            self.calls.append((name, self.decode(*args) if self.decode else args))
            return 0
        return call


def doubles(pointer, shape):
    n = int(np.prod(shape))
    return np.ctypeslib.as_array(C.cast(pointer, C.POINTER(C.c_double)), shape=(n,)).reshape(shape).copy()


class FakeCudaTensor:
    """what BatchSolver.shift asks of a torch tensor in GPU memory (no GPU here: its address is never dereferenced)"""
    is_cuda = True

    def __init__(self, shape, dtype="torch.float64", contiguous=True, index=0):
        self.shape, self.dtype, self._contiguous = tuple(shape), dtype, contiguous
        self.device = types.SimpleNamespace(index=index)

    def is_contiguous(self):
        return self._contiguous

    def data_ptr(self):
        return 0x1000


def solver(ilqg, lib, cls=None):
    s = object.__new__(cls or ilqg.BatchSolver)
    s.lib, s.h, s.B, s.N, s.device = lib, 1, B, N, 0
    s.problem = types.SimpleNamespace(nx=NX, nu=NU)
    return s


@pytest.fixture(scope="module")
def ilqg():
    return load_package().ilqg


@pytest.mark.parametrize("name", NEW)
def test_missing_entry_is_a_clear_error(ilqg, name):
    with pytest.raises(ilqg.IlqgError) as e:
        ilqg._receding_entry(OldLibrary(), name)
    assert name in str(e.value) and "rebuild" in str(e.value)


def test_methods_of_an_old_library_say_rebuild(ilqg):
    s, m = solver(ilqg, OldLibrary()), solver(ilqg, OldLibrary(), ilqg.MultiSolver)
    for call, name in ((lambda: s.head(1), "ilqg_batch_head"), (lambda: s.head(1, device=True), "ilqg_batch_head_device"),
                       (lambda: s.shift(1, FakeCudaTensor((B, NX))), "ilqg_batch_shift_device"),
                       (lambda: s.shift_param("vref", 1), "ilqg_batch_shift_param"), (lambda: m.head(1), "ilqg_multi_head")):
        with pytest.raises(ilqg.IlqgError) as e:
            call()
        assert name in str(e.value) and "rebuild" in str(e.value)


def test_host_arguments_take_the_host_entry_in_the_documented_shapes(ilqg):
    import torch
    lib = Recorder(lambda h, steps, px, pt: (h, steps, None if px is None else doubles(px, (B, NX)), None if pt is None else doubles(pt, (B, steps, NU))))
    s = solver(ilqg, lib)
    x0 = np.arange(B * NX, dtype=np.float32)  # flat and single precision: converted
    tail = np.arange(B * 3 * NU, dtype=np.float64).reshape(B, 3, NU)
    s.shift(3, x0, tail)
    s.shift(3, torch.from_numpy(x0.reshape(B, NX).astype(np.float64)), torch.from_numpy(tail))  # CPU tensors: the same way
    s.shift(2)
    assert [c[0] for c in lib.calls] == ["ilqg_batch_shift"] * 3
    for name, (h, steps, px, pt) in lib.calls[:2]:
        assert (h, steps) == (1, 3)
        assert np.array_equal(px, x0.reshape(B, NX)) and np.array_equal(pt, tail)
    assert lib.calls[2][1] == (1, 2, None, None)


def test_head_allocates_what_the_entry_fills(ilqg):
    lib = Recorder()
    s, m = solver(ilqg, lib), solver(ilqg, lib, ilqg.MultiSolver)
    h = s.head(3)
    assert sorted(h) == ["cost", "u", "x"] and h["x"].shape == (B, 3, NX) and h["u"].shape == (B, 3, NU) and h["cost"].shape == (B,)
    name, (handle, steps, x, u, l, L, cost) = lib.calls[-1]
    assert name == "ilqg_batch_head" and steps == 3 and l is None and L is None and x and u and cost
    h = m.head(2, gains=True)
    assert h["l"].shape == (B, 2, NU) and h["L"].shape == (B, 2, NU * NX)
    name, args = lib.calls[-1]
    assert name == "ilqg_multi_head" and all(a is not None for a in args)


def test_shift_param_passes_the_tail(ilqg):
    lib = Recorder(lambda h, name, steps, tail: (name, steps, None if tail is None else doubles(tail, (steps,))))
    s = solver(ilqg, lib)
    s.shift_param("vref", 3, [1, 2, 3])
    s.shift_param("vref", 3)
    (_, (name, steps, tail)), (_, last) = lib.calls
    assert name == b"vref" and steps == 3 and np.array_equal(tail, [1.0, 2.0, 3.0]) and last[2] is None
    with pytest.raises(ilqg.IlqgError) as e:
        s.shift_param("vref", 3, [1, 2])
    assert "tail" in str(e.value) and len(lib.calls) == 2


def test_device_tensors_are_checked_before_any_library_call(ilqg):
    lib = Recorder()
    s = solver(ilqg, lib)
    good = FakeCudaTensor((B, NX))
    for x0, tail, words in ((FakeCudaTensor((B, NX), dtype="torch.float32"), None, ("x0", "float64")),
                            (FakeCudaTensor((B, NX), contiguous=False), None, ("x0", "contiguous")),
                            (FakeCudaTensor((B + 1, NX)), None, ("x0", "shape")),
                            (FakeCudaTensor((B, NX), index=1), None, ("x0", "GPU")),
                            (good, FakeCudaTensor((B, 3, NU)), ("u_tail", "shape")),
                            (good, np.zeros((B, 2, NU)), ("u_tail", "host")),
                            (np.zeros((B, NX)), FakeCudaTensor((B, 2, NU)), ("x0", "host"))):
        with pytest.raises(ilqg.IlqgError) as e:
            s.shift(2, x0, tail)
        assert all(w in str(e.value) for w in words), str(e.value)
    assert lib.calls == []


def test_importing_ilqg_does_not_import_torch():
    code = ("import sys; sys.path[:0] = [%r, %r]\n"
            "from conftest import load_package\n"
            "m = load_package().ilqg\n"
            "assert hasattr(m.BatchSolver, 'head') and 'torch' not in sys.modules, sorted(k for k in sys.modules if 'torch' in k)\n"
            % (ROOT, os.path.join(ROOT, "tests")))
    subprocess.run([sys.executable, "-c", code], check=True, timeout=120)
