"""ilqg.py's side of policy_rollout(noise=(seed, sigma)) and noise_table, where no GPU is needed (in the manner of
tests/test_policy_noise_binding.py, whose stand-ins are used here): a problem library built before the _drawn entries existed
still loads, works without noise and says "rebuild" only when noise is given; noise=None calls the entries that have always
been there with the arguments they have always had; the seed, sigma as N_X C doubles, the shared flag and the first trajectory
reach the new entries, with and without a parameter table, host, device and multi; every refusal happens before any library
call; header, host code, ctypes signatures and README name the five entries."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from conftest import ROOT, load_package
from test_policy_noise_binding import NOISE, PARAMS, WithNoise, named_solver
from test_policy_rollout_binding import B, N, NX, NEW, FakeCudaTensor, OldLibrary, solver

DRAWN = ["ilqg_batch_policy_rollout_drawn", "ilqg_batch_policy_rollout_drawn_device", "ilqg_multi_policy_rollout_drawn"]
TABLE = ["ilqg_batch_noise_table", "ilqg_batch_noise_table_device"]
R = 3
SEED = (0xDEADBEEF << 32) | 0x12345678
SIGMA = [0.5, 0.0, 2.0, 1e-3]


def doubles(p, n):
    return [float(v) for v in C.cast(p, C.POINTER(C.c_double))[:n]]


class WithDrawn(WithNoise):
    """a library that has the five new entries: remembers what each was called with, sigma as values"""

    def __init__(self):
        WithNoise.__init__(self)
        for name in DRAWN:
            setattr(self, name, self._drawn_entry(name))
        for name in TABLE:
            setattr(self, name, self._table_entry(name))

    def _drawn_entry(self, name):
        def call(h, R_, x0, n_names, names, values, shared, seed, sigma, noise_shared, first, alpha, feedback, cost, ok, x_end, x, u, *stream):
            self.calls.append((name, dict(h=h, R=R_, n_names=n_names, names=None if names is None else [names[i] for i in range(n_names)],
                                          values=values, shared=shared, seed=seed, sigma=doubles(sigma, NX), noise_shared=noise_shared, first=first,
                                          alpha=alpha, feedback=feedback, out=(cost, ok, x_end, x, u), stream=stream)))
            return 0
        return call

    def _table_entry(self, name):
        def call(h, R_, seed, sigma, noise_shared, first, w, *stream):
            self.calls.append((name, dict(h=h, R=R_, seed=seed, sigma=doubles(sigma, NX), noise_shared=noise_shared, first=first, w=w, stream=stream)))
            return 0
        return call


@pytest.fixture(scope="module")
def ilqg():
    return load_package().ilqg


def test_an_old_library_works_without_noise_and_says_rebuild_with_it(ilqg):
    lib = WithNoise()  # the parent commit's entries, and none of the five
    s, m = named_solver(ilqg, lib), named_solver(ilqg, lib, ilqg.MultiSolver)
    x0 = np.zeros((B, R, NX))
    s.policy_rollout(x0)
    s.policy_rollout(x0, disturbance=np.zeros((R, N, NX)))
    m.policy_rollout(x0, params={"p": np.zeros((B, R))})
    assert [c[0] for c in lib.calls] == [NEW[0], NOISE[0], PARAMS[2]]
    for call, name in ((lambda: s.policy_rollout(x0, noise=(1, SIGMA)), DRAWN[0]),
                       (lambda: s.policy_rollout(FakeCudaTensor((B, R, NX)), device=True, noise=(1, SIGMA)), DRAWN[1]),
                       (lambda: m.policy_rollout(x0, noise=(1, SIGMA)), DRAWN[2]),
                       (lambda: s.noise_table(R, 1, SIGMA), TABLE[0]),
                       (lambda: s.noise_table(R, 1, SIGMA, device=True), TABLE[1])):
        with pytest.raises(ilqg.IlqgError) as e:
            call()
        assert name in str(e.value) and "rebuild" in str(e.value)
    assert len(lib.calls) == 3
    old = solver(ilqg, OldLibrary())
    with pytest.raises(ilqg.IlqgError) as e:
        old.policy_rollout(x0, noise=(1, SIGMA))
    assert DRAWN[0] in str(e.value) and "rebuild" in str(e.value)


def test_without_noise_the_old_entries_get_the_old_arguments(ilqg):
    lib = WithDrawn()
    s, m = named_solver(ilqg, lib), named_solver(ilqg, lib, ilqg.MultiSolver)
    x0 = np.arange(B * R * NX, dtype=np.float64).reshape(B, R, NX)
    w = np.arange(R * N * NX, dtype=np.float64).reshape(R, N, NX)
    s.policy_rollout(x0, alpha=0.25, feedback=False)
    s.policy_rollout(x0, noise=None, trajectories=True, noise_shared=True, first_trajectory=5)
    m.policy_rollout(x0, noise=None)
    s.policy_rollout(x0, params={"q": np.zeros((R, 2))}, noise=None)
    s.policy_rollout(x0, disturbance=w, noise=None)
    m.policy_rollout(x0, disturbance=w)
    assert [c[0] for c in lib.calls] == [NEW[0], NEW[0], NEW[2], PARAMS[0], NOISE[0], NOISE[2]]
    # the stand-ins' entries take exactly the parent's positional arguments: one more would have raised a TypeError
    first = lib.calls[0][1]
    assert first["R"] == R and np.array_equal(first["starts"], x0) and (first["alpha"], first["feedback"]) == (0.25, 0) and first["stream"] == ()
    assert lib.calls[3][1]["names"] == [b"q"] and lib.calls[3][1]["shared"] == 1
    assert lib.calls[4][1]["dist_shared"] == 1 and np.array_equal(lib.calls[4][1]["table"], w.ravel())


def test_seed_sigma_flag_and_first_trajectory_reach_the_entries(ilqg, monkeypatch):
    lib = WithDrawn()
    s, m = named_solver(ilqg, lib), named_solver(ilqg, lib, ilqg.MultiSolver)
    x0 = np.zeros((B, R, NX))
    s.policy_rollout(x0, noise=(SEED, SIGMA))
    s.policy_rollout(x0, alpha=0.0, feedback=False, trajectories=True, noise=(0, np.array(SIGMA, dtype=np.float32)), noise_shared=True)
    s.policy_rollout(x0, noise=(np.uint64(2 ** 64 - 1), 0.25), first_trajectory=2 ** 32 - B)
    m.policy_rollout(x0[0], noise=[7, tuple(SIGMA)], first_trajectory=np.int64(40))
    s.policy_rollout(x0, params={"q": np.ones((R, 2)), "p": np.ones(R)}, noise=(SEED, SIGMA), first_trajectory=3)
    m.policy_rollout(x0, params={"p": np.ones((B, R))}, noise=(SEED, SIGMA), noise_shared=1)
    assert [c[0] for c in lib.calls] == [DRAWN[0]] * 3 + [DRAWN[2], DRAWN[0], DRAWN[2]]
    want = [(SEED, SIGMA, 0, 0), (0, [float(np.float32(v)) for v in SIGMA], 1, 0), (2 ** 64 - 1, [0.25] * NX, 0, 2 ** 32 - B), (7, SIGMA, 0, 40),
            (SEED, SIGMA, 0, 3), (SEED, SIGMA, 1, 0)]
    for (name, c), (seed, sigma, shared, first) in zip(lib.calls, want):
        assert c["h"] == 1 and c["R"] == R and (c["seed"], c["sigma"], c["noise_shared"], c["first"]) == (seed, sigma, shared, first), name
        assert type(c["seed"]) is int and type(c["first"]) is int
    for _, c in lib.calls[:4]:  # no parameter table: n_names = 0 and nothing to read
        assert c["n_names"] == 0 and c["names"] is None and c["values"] is None and c["shared"] == 0
    assert (lib.calls[1][1]["alpha"], lib.calls[1][1]["feedback"]) == (0.0, 0) and all(p is not None for p in lib.calls[1][1]["out"])
    cost, ok, x_end, x, u = lib.calls[0][1]["out"]
    assert cost and ok and x_end and x is None and u is None
    a, b = lib.calls[4][1], lib.calls[5][1]
    assert a["names"] == [b"q", b"p"] and a["shared"] == 1 and a["values"] and b["names"] == [b"p"] and b["shared"] == 0 and b["values"]
    # the device form: the stream behind the outputs, sigma still host memory
    monkeypatch.setattr(ilqg, "_torch_stream", lambda device: (None, None, C.c_void_p(0x77)))
    monkeypatch.setattr(ilqg, "_rollout_outputs", lambda *a: ({}, [None] * 5))
    s.policy_rollout(FakeCudaTensor((B, R, NX)), device=True, alpha=0.5, noise=(SEED, SIGMA), noise_shared=True, first_trajectory=9)
    name, c = lib.calls[-1]
    assert name == DRAWN[1] and (c["seed"], c["sigma"], c["noise_shared"], c["first"]) == (SEED, SIGMA, 1, 9)
    assert c["alpha"] == 0.5 and c["n_names"] == 0 and c["stream"][0].value == 0x77


def test_noise_table_reaches_its_entry_and_has_the_documented_shape(ilqg):
    lib = WithDrawn()
    s = named_solver(ilqg, lib)
    w = s.noise_table(R, SEED, SIGMA)
    ws = s.noise_table(2, 5, 0.5, shared=True, first_trajectory=0)
    wf = s.noise_table(np.int64(1), 5, SIGMA, first_trajectory=17)
    assert w.shape == (B, R, N, NX) and ws.shape == (2, N, NX) and wf.shape == (B, 1, N, NX) and w.dtype == np.float64 and w.flags.c_contiguous
    assert [c[0] for c in lib.calls] == [TABLE[0]] * 3
    got = [(c["R"], c["seed"], c["sigma"], c["noise_shared"], c["first"]) for _, c in lib.calls]
    assert got == [(R, SEED, SIGMA, 0, 0), (2, 5, [0.5] * NX, 1, 0), (1, 5, SIGMA, 0, 17)]
    assert lib.calls[0][1]["w"].value == w.ctypes.data and lib.calls[0][1]["stream"] == ()


def test_wrong_noise_is_refused_before_any_library_call(ilqg):
    lib = WithDrawn()
    s, m = named_solver(ilqg, lib), named_solver(ilqg, lib, ilqg.MultiSolver)
    x0 = np.zeros((B, R, NX))
    bad = [(dict(noise=(1, SIGMA), disturbance=np.zeros((R, N, NX))), ("noise", "disturbance")),
           (dict(noise=7), ("noise", "(seed, sigma)")),
           (dict(noise=(1, SIGMA, 0)), ("noise", "(seed, sigma)")),
           (dict(noise=(-1, SIGMA)), ("seed",)),
           (dict(noise=(2 ** 64, SIGMA)), ("seed",)),
           (dict(noise=(1.5, SIGMA)), ("seed",)),
           (dict(noise=(True, SIGMA)), ("seed",)),
           (dict(noise=(1, SIGMA[:3])), ("sigma", "shape")),
           (dict(noise=(1, np.ones((NX, 1)))), ("sigma", "shape")),
           (dict(noise=(1, [0.5, -1e-300, 1.0, 1.0])), ("sigma", "negative")),
           (dict(noise=(1, [0.5, np.nan, 1.0, 1.0])), ("sigma", "finite")),
           (dict(noise=(1, [0.5, np.inf, 1.0, 1.0])), ("sigma", "finite")),
           (dict(noise=(1, "abcd")), ("sigma",)),
           (dict(noise=(1, FakeCudaTensor((NX,)))), ("sigma", "host")),
           (dict(noise=(1, SIGMA), first_trajectory=-1), ("first_trajectory",)),
           (dict(noise=(1, SIGMA), first_trajectory=2 ** 32 - B + 1), ("first_trajectory", "2^32")),
           (dict(noise=(1, SIGMA), first_trajectory=0.0), ("first_trajectory",))]
    for kw, words in bad:
        for q in (s, m):
            with pytest.raises(ilqg.IlqgError) as e:
                q.policy_rollout(x0, **kw)
            assert all(w in str(e.value) for w in words), (kw, str(e.value))
        if "disturbance" not in kw:
            with pytest.raises(ilqg.IlqgError) as e:
                s.policy_rollout(FakeCudaTensor((B, R, NX)), device=True, **kw)
            assert all(w in str(e.value) for w in words), (kw, str(e.value))
    with pytest.raises(ilqg.IlqgError) as e:
        s.policy_rollout(FakeCudaTensor((B, R, NX)), device=True, noise=(1, SIGMA), disturbance=FakeCudaTensor((R, N, NX)))
    assert "noise" in str(e.value) and "disturbance" in str(e.value)
    for call, words in ((lambda: s.noise_table(0, 1, SIGMA), ("R",)), (lambda: s.noise_table(2.0, 1, SIGMA), ("R",)),
                        (lambda: s.noise_table(R, -1, SIGMA), ("seed",)), (lambda: s.noise_table(R, 1, SIGMA[:2]), ("sigma", "shape")),
                        (lambda: s.noise_table(R, 1, [-1.0] * NX), ("sigma", "negative")),
                        (lambda: s.noise_table(R, 1, SIGMA, first_trajectory=2 ** 32), ("first_trajectory",)),
                        (lambda: s.noise_table(R, 1, SIGMA, first_trajectory=-3, device=True), ("first_trajectory",))):
        with pytest.raises(ilqg.IlqgError) as e:
            call()
        assert all(w in str(e.value) for w in words) and "noise_table" in str(e.value), str(e.value)
    # the starts are still checked as ever
    with pytest.raises(ilqg.IlqgError) as e:
        s.policy_rollout(np.zeros((B, R, NX + 1)), noise=(1, SIGMA))
    assert "x0" in str(e.value)
    assert lib.calls == []


def test_header_host_signatures_and_readme_name_the_five_entries(ilqg):
    header = open(os.path.join(ROOT, "include", "ilqg_batch.h")).read()
    readme = open(os.path.join(ROOT, "README.md")).read()
    host = open(os.path.join(ROOT, "ddp-generator_amd", "csrc", "ilqg_host.c")).read()
    src = open(os.path.join(ROOT, "ddp-generator_amd", "ilqg.py")).read()
    for name in DRAWN + TABLE:
        assert re.search(r"^int %s\(" % name, header, re.M), name
        assert re.search(r"^int %s\(" % name, host, re.M), name
        assert name in readme, name
        assert "lib.%s.argtypes" % name in src, name

    def args(name):
        decl = re.search(r"^int %s\((.*?)\);" % name, header, re.M | re.S).group(1)
        return [a.strip().split()[-1].lstrip("*") for a in decl.replace("\n", " ").split(",")]
    # the argument list of the _noise form with `disturbance, disturbance_shared` replaced
    noise = args("ilqg_batch_policy_rollout_noise")
    at = noise.index("disturbance")
    want = noise[:at] + ["seed", "sigma", "noise_shared", "first_trajectory"] + noise[at + 2:]
    assert args(DRAWN[0]) == want and args(DRAWN[1]) == want + ["stream"] and args(DRAWN[2]) == ["m"] + want[1:]
    assert args(TABLE[0]) == ["c", "n_starts", "seed", "sigma", "noise_shared", "first_trajectory", "w"] and args(TABLE[1]) == args(TABLE[0]) + ["stream"]
    assert re.search(r"unsigned long long seed, const double \*sigma, int noise_shared,\s+long long first_trajectory", header)
    v, i, d = "v", "C.c_int", "C.c_double"
    want = ", ".join([v, i, v, i, "C.POINTER(C.c_char_p)", v, i, "C.c_ulonglong", v, i, "C.c_longlong", d, i, v, v, v, v, v])
    assert "drawn = [%s]" % want in src
    assert "lib.ilqg_batch_noise_table.argtypes = [v, C.c_int, C.c_ulonglong, v, C.c_int, C.c_longlong, v]" in src
