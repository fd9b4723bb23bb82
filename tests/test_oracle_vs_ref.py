"""The CPU restatement against the reference build on fresh seeded inputs — exact equality, beyond the committed
fixtures of tests/test_oracle_golden.py.  What the reference's own solver sources computed on these inputs is stored in
tests/golden/oracle_vs_ref.npz (tests/golden/make_goldens.py vsref), so the comparison runs everywhere; where the
reference build oracle/_ref exists, the oracle is compared with it live as well."""
import os

import numpy as np
import pytest

from conftest import golden, load_package, ref_available
from oracle.harness import CAR_PARAMS, CONSOLE_CASES, Driver, Kernels, console_of, lib_path

SOLVE_KEYS = ("rc", "x", "u", "l", "L")


def solve_outputs(lib, fd):
    """60-iteration solves of three seeded CarParking starts: return code, scalars, trajectory, gains, trace"""
    synth = load_package().synth
    x0s, u0s = synth.car_batch(3, first=5000)
    out = {}
    for b in range(3):
        d = Driver(lib, 500, CAR_PARAMS, dict(max_iter=60))
        assert d.init(x0s[b], u0s[b]) == 1
        out["%d/rc" % b] = np.array(d.solve())
        for k, v in d.scalars().items():
            out["%d/scalar/%s" % (b, k)] = np.array(v)
        out["%d/x" % b], out["%d/u" % b] = d.traj(0)
        out["%d/l" % b], out["%d/L" % b] = d.gains()
        for k, v in d.trace().items():
            out["%d/trace/%s" % (b, k)] = np.asarray(v)
        d.close()
    return out


def boxqp_outputs(K):
    """300 random box QPs of size 1..8, positive definite Hessians (rc -2, which prints, is avoided)"""
    rng = np.random.default_rng(7)
    rc, n_free, x, clamp = [], [], [], []
    for trial in range(300):
        n = int(rng.integers(1, 9))
        A = rng.standard_normal((n, n))
        M = A @ A.T + 10.0 ** rng.uniform(-6, 0) * np.eye(n)
        H = np.array([M[r, c] for c in range(n) for r in range(c + 1)])
        g = rng.standard_normal(n)
        lo = -np.abs(rng.standard_normal(n)); hi = np.abs(rng.standard_normal(n))
        x0 = rng.standard_normal(n)
        a = K.boxqp(H, g, lo, hi, x0)
        rc.append(a["rc"]); n_free.append(a["n_free"]); x.append(np.asarray(a["x"], dtype=np.float64)); clamp.append(np.asarray(a["clamp"]))
    return {"rc": np.array(rc), "n_free": np.array(n_free), "x": np.concatenate(x), "clamp": np.concatenate(clamp)}


def dense_outputs(K):
    """cholesky_tri / cholesky_tri_inv / addMulVec / addSquareTri / addMul2Tri on 200 random inputs of size 1..16"""
    rng = np.random.default_rng(11)
    ok, parts = [], {k: [] for k in ("U", "Uinv", "mul_vec", "square_uu", "square_xx", "mul2")}
    for trial in range(200):
        n = int(rng.integers(1, 17))
        A = rng.standard_normal((n, n))
        M = A @ A.T + 10.0 ** rng.uniform(-8, 0) * np.eye(n) if trial % 3 else (A + A.T) / 2
        P = np.array([M[r, c] for c in range(n) for r in range(c + 1)])
        okc, U = K.cholesky(P, n)
        ok.append(okc)
        if okc:
            parts["U"].append(np.asarray(U, dtype=np.float64)); parts["Uinv"].append(np.asarray(K.cholesky_inv(U, n), dtype=np.float64))
        m = int(rng.integers(1, n + 1))
        V = np.array([(A @ A.T)[r, c] for c in range(n) for r in range(c + 1)])
        fx, fu, vx = rng.standard_normal(n * n), rng.standard_normal(n * m), rng.standard_normal(n)
        rng.standard_normal(m)  # (a draw the inputs have always skipped)
        parts["mul_vec"].append(K.add_mul_vec(np.full(m, 1.5), vx, fu, n, m))
        b_uu, b_xx, b_xu = rng.standard_normal(m * (m + 1) // 2), rng.standard_normal(n * (n + 1) // 2), rng.standard_normal(n * m)
        parts["square_uu"].append(K.add_square_tri(b_uu, V, fu, n, m))
        parts["square_xx"].append(K.add_square_tri(b_xx, V, fx, n, n))
        parts["mul2"].append(K.add_mul2_tri(b_xu, V, fx, n, n, fu, n, m))
    out = {k: np.concatenate([np.ravel(np.asarray(a, dtype=np.float64)) for a in v]) for k, v in parts.items()}
    out["ok"] = np.array(ok, dtype=np.int32)
    return out


def stored(prefix):
    g = golden("oracle_vs_ref.npz")
    return {k[len(prefix):]: g[k] for k in g.files if k.startswith(prefix)}


def assert_same(got, want):
    assert sorted(got) == sorted(want)
    for k in want:
        assert np.array_equal(np.asarray(got[k]), want[k]), k


@pytest.mark.parametrize("fd", [0, 1])
def test_randomised_solves_match_reference(oracle_built, fd):
    o = solve_outputs(lib_path("oracle", full_ddp=fd), fd)
    assert_same(o, stored("solves_fd%d/" % fd))
    if ref_available(fd):
        assert_same(o, solve_outputs(lib_path("ref", full_ddp=fd), fd))


def test_random_boxqp_match_reference(oracle_built):
    o = boxqp_outputs(Kernels(lib_path("oracle")))
    assert_same(o, stored("boxqp/"))
    if ref_available():
        assert_same(o, boxqp_outputs(Kernels(lib_path("ref"))))


def test_dense_helpers_match_the_reference_built_without_any_stand_in(oracle_built):
    """cholesky.c, matMult.c and printMat.c are the reference files that include neither mex.h nor a generated header:
    _ref/libref_pure.so is those three compiled with nothing but -I<reference> -DPRNT=printf (the stored vectors come from
    it).  The restatement's cholesky_tri / cholesky_tri_inv / addMulVec / addSquareTri / addMul2Tri equal it exactly on
    fresh inputs."""
    o = dense_outputs(Kernels(lib_path("oracle")))
    assert_same(o, stored("dense/"))
    if os.path.exists(lib_path("pure")):
        assert_same(o, dense_outputs(Kernels(lib_path("pure"))))


@pytest.mark.parametrize("problem,fd", CONSOLE_CASES)
def test_console_fixture_is_what_the_reference_prints(oracle_built, problem, fd):
    """tests/golden/trace_*.txt (the iteration lines the product's iLQG() is compared with on the GPU,
    tests/test_gpu_dropin.py) are the reference's own console output with its default switches"""
    lib = os.path.join(os.path.dirname(lib_path("ref")), "libref_%s_fd%d_trace.so" % (problem, fd))
    if not os.path.exists(lib):
        pytest.skip("trace build of the reference not present")
    with open(os.path.join(os.path.dirname(__file__), "golden", "trace_%s_fd%d.txt" % (problem, fd))) as f:
        assert console_of(lib, problem, fd) == f.read()
