"""ilqg.py's side of policy_rollout(disturbance=...), where no GPU is needed (in the manner of
tests/test_policy_rollout_binding.py, whose stand-ins are used here): a problem library built before the _noise entries existed
still loads, works without a disturbance and says "rebuild" only when one is given; disturbance=None calls the entries that
have always been there with the arguments they have always had; a table [B,R,N,nx] / [R,N,nx] reaches the superset entry as
C-contiguous doubles with the right disturbance_shared, with and without a parameter table; wrong shapes, dtypes, devices and
non-contiguous tensors are refused before any library call; header, ctypes signatures and README name the three entries."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from conftest import ROOT, load_package
from test_policy_rollout_binding import B, N, NX, NU, NEW, FakeCudaTensor, OldLibrary, Recorder, solver

NOISE = ["ilqg_batch_policy_rollout_noise", "ilqg_batch_policy_rollout_noise_device", "ilqg_multi_policy_rollout_noise"]
PARAMS = ["ilqg_batch_policy_rollout_params", "ilqg_batch_policy_rollout_params_device", "ilqg_multi_policy_rollout_params"]
R = 3


class BeforeNoise(Recorder):
    """a library with the roll-out entries of the parent commit, and no _noise entry"""

    def __init__(self):
        Recorder.__init__(self)
        for name in PARAMS:
            setattr(self, name, self._params_entry(name))

    def _params_entry(self, name):
        def call(h, R_, x0, n_names, names, values, shared, alpha, feedback, cost, ok, x_end, x, u, *stream):
            self.calls.append((name, dict(h=h, R=R_, n_names=n_names, names=[names[i] for i in range(n_names)], shared=shared, alpha=alpha,
                                          feedback=feedback, out=(cost, ok, x_end, x, u), stream=stream)))
            return 0
        return call


class WithNoise(BeforeNoise):
    """a library that has the three _noise entries: remembers what each was called with, the table as values"""

    def __init__(self):
        BeforeNoise.__init__(self)
        for name in NOISE:
            setattr(self, name, self._noise_entry(name))

    def _noise_entry(self, name):
        def call(h, R_, x0, n_names, names, values, shared, dist, dist_shared, alpha, feedback, cost, ok, x_end, x, u, *stream):
            table = None
            if not name.endswith("_device"):
                n = (R_ if dist_shared else B * R_) * N * NX
                table = np.ctypeslib.as_array(C.cast(dist, C.POINTER(C.c_double)), shape=(n,)).copy()
            self.calls.append((name, dict(h=h, R=R_, n_names=n_names, names=None if names is None else [names[i] for i in range(n_names)],
                                          values=values, shared=shared, dist=dist, table=table, dist_shared=dist_shared, alpha=alpha,
                                          feedback=feedback, out=(cost, ok, x_end, x, u), stream=stream)))
            return 0
        return call


def named_solver(ilqg, lib, cls=None):
    s = solver(ilqg, lib, cls)
    s.problem.params = [("p", 1), ("q", 2), ("track", -1)]
    return s


@pytest.fixture(scope="module")
def ilqg():
    return load_package().ilqg


def test_an_old_library_works_without_a_disturbance_and_says_rebuild_with_one(ilqg):
    lib = BeforeNoise()
    s, m = named_solver(ilqg, lib), named_solver(ilqg, lib, ilqg.MultiSolver)
    x0, w = np.zeros((B, R, NX)), np.zeros((B, R, N, NX))
    s.policy_rollout(x0)
    m.policy_rollout(x0, params={"p": np.zeros((B, R))})
    assert [c[0] for c in lib.calls] == [NEW[0], PARAMS[2]]
    for call, name in ((lambda: s.policy_rollout(x0, disturbance=w), NOISE[0]),
                       (lambda: s.policy_rollout(FakeCudaTensor((B, R, NX)), device=True, disturbance=FakeCudaTensor((B, R, N, NX))), NOISE[1]),
                       (lambda: m.policy_rollout(x0, disturbance=w[0]), NOISE[2])):
        with pytest.raises(ilqg.IlqgError) as e:
            call()
        assert name in str(e.value) and "rebuild" in str(e.value)
    assert len(lib.calls) == 2
    old = solver(ilqg, OldLibrary())
    with pytest.raises(ilqg.IlqgError) as e:
        old.policy_rollout(x0, disturbance=w)
    assert NOISE[0] in str(e.value) and "rebuild" in str(e.value)


def test_without_a_disturbance_the_old_entries_get_the_old_arguments(ilqg):
    lib = WithNoise()
    s, m = named_solver(ilqg, lib), named_solver(ilqg, lib, ilqg.MultiSolver)
    x0 = np.arange(B * R * NX, dtype=np.float64).reshape(B, R, NX)
    s.policy_rollout(x0, alpha=0.25, feedback=False)
    s.policy_rollout(x0, disturbance=None, trajectories=True)
    m.policy_rollout(x0, disturbance=None)
    s.policy_rollout(x0, params={"q": np.zeros((R, 2))}, disturbance=None)
    m.policy_rollout(x0, params={"p": np.zeros((B, R))})
    assert [c[0] for c in lib.calls] == [NEW[0], NEW[0], NEW[2], PARAMS[0], PARAMS[2]]
    # the Recorder's entries take exactly the parent's positional arguments: one more would have raised a TypeError
    first = lib.calls[0][1]
    assert first["R"] == R and np.array_equal(first["starts"], x0) and (first["alpha"], first["feedback"]) == (0.25, 0) and first["stream"] == ()
    assert all(p is not None for p in lib.calls[1][1]["out"])
    assert lib.calls[3][1]["names"] == [b"q"] and lib.calls[3][1]["shared"] == 1 and lib.calls[4][1]["shared"] == 0


def test_tables_reach_the_entry_in_the_documented_shape(ilqg):
    lib = WithNoise()
    s, m = named_solver(ilqg, lib), named_solver(ilqg, lib, ilqg.MultiSolver)
    x0 = np.zeros((B, R, NX))
    full = np.arange(B * R * N * NX, dtype=np.float64).reshape(B, R, N, NX)
    short = np.arange(R * N * NX, dtype=np.float32).reshape(R, N, NX)     # single precision, one table for every trajectory
    strided = np.zeros((B, R, N, 2 * NX))[..., ::2] + full                # not contiguous: copied
    s.policy_rollout(x0, disturbance=full)
    s.policy_rollout(x0, alpha=0.0, feedback=False, disturbance=short, trajectories=True)
    s.policy_rollout(x0, disturbance=strided)
    m.policy_rollout(x0, disturbance=full)
    m.policy_rollout(x0[0], disturbance=short)
    s.policy_rollout(x0, params={"q": np.ones((R, 2)), "p": np.ones(R)}, disturbance=full)
    m.policy_rollout(x0, params={"p": np.ones((B, R))}, disturbance=short)
    assert [c[0] for c in lib.calls] == [NOISE[0]] * 3 + [NOISE[2]] * 2 + [NOISE[0], NOISE[2]]
    want = [(full, 0), (short, 1), (full, 0), (full, 0), (short, 1), (full, 0), (short, 1)]
    for (name, c), (w, sh) in zip(lib.calls, want):
        assert c["h"] == 1 and c["R"] == R and c["dist_shared"] == sh and np.array_equal(c["table"], w.astype(np.float64).ravel()), name
    for _, c in lib.calls[:5]:  # no parameter table: n_names = 0 and nothing to read
        assert c["n_names"] == 0 and c["names"] is None and c["values"] is None and c["shared"] == 0
    assert (lib.calls[1][1]["alpha"], lib.calls[1][1]["feedback"]) == (0.0, 0) and all(p is not None for p in lib.calls[1][1]["out"])
    cost, ok, x_end, x, u = lib.calls[0][1]["out"]
    assert cost and ok and x_end and x is None and u is None
    a, b = lib.calls[5][1], lib.calls[6][1]
    assert a["names"] == [b"q", b"p"] and a["shared"] == 1 and a["values"] and b["names"] == [b"p"] and b["shared"] == 0 and b["values"]
    # R = B: a [B, N, nx] table is the shared form of R = B roll-outs, a [B, B, N, nx] one the full form
    s.policy_rollout(np.zeros((B, B, NX)), disturbance=np.zeros((B, N, NX)))
    s.policy_rollout(np.zeros((B, B, NX)), disturbance=np.zeros((B, B, N, NX)))
    assert [c[1]["dist_shared"] for c in lib.calls[-2:]] == [1, 0]


def test_a_device_table_is_read_where_it_is(ilqg, monkeypatch):
    lib = WithNoise()
    s = named_solver(ilqg, lib)
    monkeypatch.setattr(ilqg, "_torch_stream", lambda device: (None, None, C.c_void_p(0x77)))
    monkeypatch.setattr(ilqg, "_rollout_outputs", lambda *a: ({}, [None] * 5))
    x0 = FakeCudaTensor((B, R, NX))
    s.policy_rollout(x0, device=True, disturbance=FakeCudaTensor((B, R, N, NX)))
    s.policy_rollout(x0, device=True, disturbance=FakeCudaTensor((R, N, NX)), alpha=0.5)
    s.policy_rollout(x0, device=True)
    assert [c[0] for c in lib.calls] == [NOISE[1], NOISE[1], NEW[1]]
    for (_, c), sh in zip(lib.calls[:2], (0, 1)):
        assert c["dist"].value == 0x1000 and c["dist_shared"] == sh and c["n_names"] == 0 and c["names"] is None and c["stream"][0].value == 0x77
    assert lib.calls[1][1]["alpha"] == 0.5


def test_wrong_tables_are_refused_before_any_library_call(ilqg):
    import torch
    lib = WithNoise()
    s, m = named_solver(ilqg, lib), named_solver(ilqg, lib, ilqg.MultiSolver)
    x0 = np.zeros((B, R, NX))
    for w in (np.zeros((B, R, N + 1, NX)), np.zeros((B, R, N, NX + 1)), np.zeros((B, R + 1, N, NX)), np.zeros((B + 1, R, N, NX)), np.zeros((N, NX)),
              np.zeros((R, N)), np.zeros((B, R, N, NX, 1)), np.zeros(0)):
        for q in (s, m):
            with pytest.raises(ilqg.IlqgError) as e:
                q.policy_rollout(x0, disturbance=w)
            assert "disturbance" in str(e.value) and "shape" in str(e.value)
    for w, words in ((np.zeros((R, N, NX), dtype=complex), ("disturbance", "dtype")),
                     (np.full((R, N, NX), "a"), ("disturbance", "dtype")),
                     (FakeCudaTensor((R, N, NX)), ("disturbance", "device=True"))):
        for q in (s, m):
            with pytest.raises(ilqg.IlqgError) as e:
                q.policy_rollout(x0, disturbance=w)
            assert all(word in str(e.value) for word in words), str(e.value)
    good = FakeCudaTensor((B, R, NX))
    for w, words in ((FakeCudaTensor((R, N, NX), dtype="torch.float32"), ("disturbance", "float64")),
                     (FakeCudaTensor((B, R, N, NX), contiguous=False), ("disturbance", "contiguous")),
                     (FakeCudaTensor((B, R, N, NX + 1)), ("disturbance", "shape")),
                     (FakeCudaTensor((B, R + 1, N, NX)), ("disturbance", "shape")),
                     (FakeCudaTensor((N, NX)), ("disturbance", "shape")),
                     (FakeCudaTensor((R, N, NX), index=1), ("disturbance", "GPU")),
                     (np.zeros((R, N, NX)), ("disturbance", "host")),
                     (torch.zeros((B, R, N, NX), dtype=torch.float64), ("disturbance", "host"))):
        with pytest.raises(ilqg.IlqgError) as e:
            s.policy_rollout(good, device=True, disturbance=w)
        assert all(word in str(e.value) for word in words), str(e.value)
    assert lib.calls == []


def test_header_signatures_and_readme_name_the_three_entries(ilqg):
    header = open(os.path.join(ROOT, "include", "ilqg_batch.h")).read()
    readme = open(os.path.join(ROOT, "README.md")).read()
    host = open(os.path.join(ROOT, "ddp-generator_amd", "csrc", "ilqg_host.c")).read()
    for name in NOISE:
        assert re.search(r"^int %s\(" % name, header, re.M), name
        assert re.search(r"^int %s\(" % name, host, re.M), name
        assert name in readme, name
    # the ctypes signatures: 16 arguments in the order of the header, the device form with the stream behind them
    src = open(os.path.join(ROOT, "ddp-generator_amd", "ilqg.py")).read()
    for name in NOISE:
        assert "lib.%s.argtypes" % name in src, name
    decl = re.search(r"^int ilqg_batch_policy_rollout_noise\((.*?)\);", header, re.M | re.S).group(1)
    args = [a.strip().split()[-1].lstrip("*") for a in decl.replace("\n", " ").split(",")]
    assert args == ["c", "n_starts", "x0", "n_names", "names", "values", "shared", "disturbance", "disturbance_shared", "alpha", "feedback",
                    "cost", "ok", "x_end", "x", "u"]
    v, i, d = "v", "C.c_int", "C.c_double"
    want = ", ".join([v, i, v, i, "C.POINTER(C.c_char_p)", v, i, v, i, d, i, v, v, v, v, v])
    assert "noise = [%s]" % want in src
