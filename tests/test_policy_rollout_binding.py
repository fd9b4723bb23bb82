"""ilqg.py's side of BatchSolver.policy_rollout / MultiSolver.policy_rollout, where no GPU is needed: a problem library built
before the entries existed still loads and says "rebuild" when they are asked for; the starts reach the host entry as
[B, R, nx] C-contiguous doubles, given so or as [R, nx] for every trajectory; the outputs have the documented shapes and
types; a tensor on the device is checked BEFORE any library call; and importing ilqg does not import torch."""
import ctypes as C
import os
import subprocess
import sys
import types

import numpy as np
import pytest

from conftest import ROOT, load_package

NEW = ["ilqg_batch_policy_rollout", "ilqg_batch_policy_rollout_device", "ilqg_multi_policy_rollout"]
B, N, NX, NU = 5, 12, 4, 2


class OldLibrary:
    """stands for a CDLL without the new symbols"""


class Recorder:
    """stands for a library that has them: remembers what each entry was called with, the starts as values"""

    def __init__(self):
        self.calls = []
        for name in NEW:
            setattr(self, name, self._entry(name))

    def _entry(self, name):
        def call(h, R, x0, alpha, feedback, cost, ok, x_end, x, u, *stream):
            starts = None
            if name != "ilqg_batch_policy_rollout_device":
                starts = np.ctypeslib.as_array(C.cast(x0, C.POINTER(C.c_double)), shape=(B * R * NX,)).reshape(B, R, NX).copy()
            self.calls.append((name, dict(h=h, R=R, x0=x0, starts=starts, alpha=alpha, feedback=feedback, out=(cost, ok, x_end, x, u), stream=stream)))
            return 0
        return call


class FakeCudaTensor:
    """what policy_rollout asks of a torch tensor in GPU memory (no GPU here: its address is never dereferenced)"""
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


def test_methods_of_an_old_library_say_rebuild(ilqg):
    s, m = solver(ilqg, OldLibrary()), solver(ilqg, OldLibrary(), ilqg.MultiSolver)
    x0 = np.zeros((B, 3, NX))
    for call, name in ((lambda: s.policy_rollout(x0), NEW[0]), (lambda: s.policy_rollout(FakeCudaTensor((B, 3, NX)), device=True), NEW[1]),
                       (lambda: m.policy_rollout(x0), NEW[2])):
        with pytest.raises(ilqg.IlqgError) as e:
            call()
        assert name in str(e.value) and "rebuild" in str(e.value)


def test_starts_reach_the_entry_in_the_documented_shape(ilqg):
    import torch
    lib = Recorder()
    s, m = solver(ilqg, lib), solver(ilqg, lib, ilqg.MultiSolver)
    full = np.arange(B * 3 * NX, dtype=np.float64).reshape(B, 3, NX)
    shared = np.arange(3 * NX, dtype=np.float32).reshape(3, NX)  # single precision, one set for every trajectory
    strided = np.zeros((B, 3, 2 * NX))[:, :, ::2] + full          # not contiguous: copied
    s.policy_rollout(full)
    s.policy_rollout(shared, alpha=0.25, feedback=False)
    s.policy_rollout(strided, alpha=0)
    s.policy_rollout(torch.from_numpy(full))  # a CPU tensor: the host entry
    m.policy_rollout(shared, trajectories=True)
    names = [c[0] for c in lib.calls]
    assert names == [NEW[0]] * 4 + [NEW[2]]
    want = [full, np.broadcast_to(shared.astype(np.float64), (B, 3, NX)), full, full, np.broadcast_to(shared.astype(np.float64), (B, 3, NX))]
    for (name, c), w in zip(lib.calls, want):
        assert c["h"] == 1 and c["R"] == 3 and np.array_equal(c["starts"], w), name
    assert [(c["alpha"], c["feedback"]) for _, c in lib.calls] == [(1.0, 1), (0.25, 0), (0.0, 1), (1.0, 1), (1.0, 1)]
    # costs only: no pointer for the whole roll-outs; with trajectories all five
    cost, ok, x_end, x, u = lib.calls[0][1]["out"]
    assert cost and ok and x_end and x is None and u is None
    assert all(p is not None for p in lib.calls[4][1]["out"])


def test_outputs_have_the_documented_shapes(ilqg):
    s = solver(ilqg, Recorder())
    out = s.policy_rollout(np.zeros((2, NX)))
    assert sorted(out) == ["cost", "ok", "x_end"]
    assert out["cost"].shape == (B, 2) and out["ok"].shape == (B, 2) and out["ok"].dtype == np.int32 and out["x_end"].shape == (B, 2, NX)
    out = s.policy_rollout(np.zeros((B, 1, NX)), trajectories=True)
    assert out["x"].shape == (B, 1, N + 1, NX) and out["u"].shape == (B, 1, N, NU)
    assert all(a.flags["C_CONTIGUOUS"] for a in out.values()) and all(out[k].dtype == np.float64 for k in ("cost", "x_end", "x", "u"))


def test_wrong_starts_are_refused_before_any_library_call(ilqg):
    lib = Recorder()
    s, m = solver(ilqg, lib), solver(ilqg, lib, ilqg.MultiSolver)
    for x0 in (np.zeros((B, 0, NX)), np.zeros((0, NX)), np.zeros((B + 1, 3, NX)), np.zeros((B, 3, NX + 1)), np.zeros(NX), np.zeros((3, NX + 1)),
               np.zeros((B, 3, NX, 1))):
        for q in (s, m):
            with pytest.raises(ilqg.IlqgError) as e:
                q.policy_rollout(x0)
            assert "x0" in str(e.value) and "shape" in str(e.value) and "n_starts" in str(e.value)
    with pytest.raises(ilqg.IlqgError) as e:
        s.policy_rollout(FakeCudaTensor((B, 3, NX)))  # a device tensor without device=True
    assert "x0" in str(e.value) and "device=True" in str(e.value)
    assert lib.calls == []


def test_device_tensors_are_checked_before_any_library_call(ilqg):
    import torch
    lib = Recorder()
    s = solver(ilqg, lib)
    for x0, words in ((FakeCudaTensor((B, 3, NX), dtype="torch.float32"), ("x0", "float64")),
                      (FakeCudaTensor((B, 3, NX), contiguous=False), ("x0", "contiguous")),
                      (FakeCudaTensor((B + 1, 3, NX)), ("x0", "shape")),
                      (FakeCudaTensor((B, 3, NX + 1)), ("x0", "shape")),
                      (FakeCudaTensor((3, NX)), ("x0", "shape")),
                      (FakeCudaTensor((B, 0, NX)), ("x0", "n_starts")),
                      (FakeCudaTensor((B, 3, NX), index=1), ("x0", "GPU")),
                      (np.zeros((B, 3, NX)), ("x0", "host")),
                      (torch.zeros((B, 3, NX), dtype=torch.float64), ("x0", "host"))):
        with pytest.raises(ilqg.IlqgError) as e:
            s.policy_rollout(x0, device=True)
        assert all(w in str(e.value) for w in words), str(e.value)
    assert lib.calls == []


def test_importing_ilqg_does_not_import_torch():
    code = ("import sys; sys.path[:0] = [%r, %r]\n"
            "from conftest import load_package\n"
            "m = load_package().ilqg\n"
            "assert hasattr(m.BatchSolver, 'policy_rollout') and hasattr(m.MultiSolver, 'policy_rollout')\n"
            "assert 'torch' not in sys.modules, sorted(k for k in sys.modules if 'torch' in k)\n"
            % (ROOT, os.path.join(ROOT, "tests")))
    subprocess.run([sys.executable, "-c", code], check=True, timeout=120)
