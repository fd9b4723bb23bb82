"""TEST INFRASTRUCTURE — one generator of box-QP problems for every device form of boxQP.c (box_qp, box_qp_row,
box_qp_rows, box_qp_quad), the reference's own boxQP on them, and the orders in which the quad form's four rows of a
wavefront meet them.  tests/test_boxqp_cases_recipe.py pins the generator to the reference build (no GPU);
tests/test_gpu_boxqp_forms.py uses it.

cases(n, seed) draws, in this order (H packed as the reference stores it: entry (r, c), r <= c, at c (c + 1) / 2 + r):
    rand        240  A A' + 10^U(-8, 0) I; g, x0 standard normal; lo = -|N|, hi = |N|
    well        120  as rand, ridge 1e-3 (tests/test_gpu_parity.py test_boxqp_random_vs_oracle)
    indef        40  A A' - 2 I
    scale       120  as rand, H and g times 2^-260, 2^-150, 2^150, 2^260 (30 each; tags scale-260 ... scale+260): the
                     device forms' short sqrt / reciprocal / quotient hold for pivots in [2^-200, 2^200]
    allclamp     40  A A' + I; |g| = 50 (1 + |N|) with random signs
    degenerate   40  ridge 1e-3; one variable with lo == hi; x0 = 10 N (outside the box)
    zero         20  A A' + I; g = 0; x0 = 0; box [-1, 1]
    singular     40  v v' + 10^U(-16, -11) I; box of width about 1e3
and for n = 2 and n = 8 the goldens of tests/golden/kernels.npz behind them (tag golden).

Exit codes of the reference's boxQP (FMA-free build) on cases(n, SEED[n]), goldens left out:
    n    -2   -1    1    2    4    5    6
    1     7   21    -    9    1  254  368
    2    20   35    -    9    3  399  194
    3    29   33    -   16   11  490   81
    8    20   46    1   30   12  512   39
(the goldens add every code, 1 included, at n = 2 and 8).  No `well` case was replaced: none disagrees with the reference
in the product builds (tests/test_gpu_boxqp_forms.py).
"""
import ctypes as C
import os

import numpy as np

from oracle.harness import Kernels, lib_path

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "kernels.npz")

SEED = {1: 101, 2: 102, 3: 103, 8: 108}
SCALES = (("scale-260", -260.0), ("scale-150", -150.0), ("scale+150", 150.0), ("scale+260", 260.0))
# families whose pivots leave the short forms' range, or whose factorisation fails: in `mixed` each of these problems
# sits beside three problems of the plain range
OUT_OF_RANGE = ("scale-260", "scale+260")
APART = OUT_OF_RANGE + ("indef",)
# the product build (FMA contraction) is held to the reference on these; the ill-conditioned and scaled families take
# their exits at rounding resolution (tests/test_gpu_parity.py test_boxqp_golden) and are held bit for bit in the
# FMA-free builds
PRODUCT_FAMILIES = ("well", "allclamp", "degenerate", "zero", "indef")


def tri(n):
    return n * (n + 1) // 2


def pack(M):
    """[count, n, n] symmetric -> [count, tri(n)], the reference's packed upper triangle"""
    n = M.shape[-1]
    return np.ascontiguousarray(np.stack([M[:, r, c] for c in range(n) for r in range(c + 1)], axis=1))


def unpack(H, n):
    M = np.zeros((n, n))
    for c in range(n):
        for r in range(c + 1):
            M[r, c] = M[c, r] = H[c * (c + 1) // 2 + r]
    return M


def cases(n, seed=None):
    """dict(H [P, tri(n)], g, lo, hi, x0 [P, n], family [P] of str, golden [P]: index into kernels.npz or -1)"""
    rng = np.random.default_rng(SEED[n] if seed is None else seed)
    eye = np.eye(n)
    parts = []

    def gram(count):
        A = rng.standard_normal((count, n, n))
        return A @ np.transpose(A, (0, 2, 1))

    def box(count):
        return -np.abs(rng.standard_normal((count, n))), np.abs(rng.standard_normal((count, n)))

    def rand(count, ridge=None):
        M = gram(count)
        r = 10.0 ** rng.uniform(-8, 0, count) if ridge is None else np.full(count, ridge)
        M = M + r[:, None, None] * eye
        g, x0 = rng.standard_normal((count, n)), rng.standard_normal((count, n))
        lo, hi = box(count)
        return M, g, lo, hi, x0

    def add(tag, M, g, lo, hi, x0):
        parts.append((np.full(len(M), tag, dtype=object), pack(M), g, lo, hi, x0))

    add("rand", *rand(240))
    add("well", *rand(120, 1e-3))
    M, g, lo, hi, x0 = rand(40, 0.0)
    add("indef", M - 2.0 * eye, g, lo, hi, x0)
    for tag, e in SCALES:
        M, g, lo, hi, x0 = rand(30)
        add(tag, M * 2.0 ** e, g * 2.0 ** e, lo, hi, x0)
    M, g, lo, hi, x0 = rand(40, 1.0)
    g = 50.0 * (1.0 + np.abs(g)) * rng.choice([-1.0, 1.0], (40, n))
    add("allclamp", M, g, lo, hi, x0)
    M, g, lo, hi, x0 = rand(40, 1e-3)
    k = rng.integers(0, n, 40)
    hi[np.arange(40), k] = lo[np.arange(40), k]
    add("degenerate", M, g, lo, hi, 10.0 * x0)
    add("zero", gram(20) + eye, np.zeros((20, n)), -np.ones((20, n)), np.ones((20, n)), np.zeros((20, n)))
    v = rng.standard_normal((40, n))
    M = v[:, :, None] * v[:, None, :] + (10.0 ** rng.uniform(-16, -11, 40))[:, None, None] * eye
    w = 500.0 * (0.5 + rng.uniform(0, 1, (2, 40, n)))
    add("singular", M, rng.standard_normal((40, n)), -w[0], w[1], rng.standard_normal((40, n)))

    gold = [np.full(len(p[0]), -1) for p in parts]
    if n in (2, 8):
        G = np.load(GOLDEN)
        sel = np.nonzero(G["qp_n"] == n)[0]
        t = tri(n)
        parts.append((np.full(len(sel), "golden", dtype=object), G["qp_H"][sel][:, :t], G["qp_g"][sel][:, :n], G["qp_lo"][sel][:, :n],
                      G["qp_hi"][sel][:, :n], G["qp_x0"][sel][:, :n]))
        gold.append(sel)
    cat = lambda i: np.ascontiguousarray(np.concatenate([p[i] for p in parts]))
    return dict(n=n, family=cat(0), H=cat(1), g=cat(2), lo=cat(3), hi=cat(4), x0=cat(5), golden=np.concatenate(gold).astype(np.int64))


_ref = {}


def reference(n, seed=None):
    """(cases(n, seed), the reference's boxQP on every one of them: rc [P], x [P, n], clamp [P, n], n_free [P]) — computed
    once per process.  boxQP is size-generic: any problem's reference build exports it.  (The reference prints H on its
    exit -2: that text on stdout is expected.)"""
    key = (n, seed)
    if key not in _ref:
        c = cases(n, seed)
        K = Kernels(lib_path("ref", "carparking", 0))
        P = len(c["H"])
        out = dict(rc=np.zeros(P, dtype=np.int32), x=np.zeros((P, n)), clamp=np.zeros((P, n), dtype=np.int32), n_free=np.zeros(P, dtype=np.int32))
        for i in range(P):
            o = K.boxqp(c["H"][i], c["g"][i], c["lo"][i], c["hi"][i], c["x0"][i])
            out["rc"][i], out["x"][i], out["clamp"][i], out["n_free"][i] = o["rc"], o["x"], o["clamp"], o["n_free"]
        C.CDLL(None).fflush(None)  # (what the reference printed leaves C's buffer now, not when the process ends)
        _ref[key] = (c, out)
    return _ref[key]


def packings(rc_ref, n_problems, family):
    """Orders in which the quad form (four problems per wavefront: slots 4 w ... 4 w + 3 are the rows of wavefront w) meets
    the problems:
        sorted  index order by the reference's code: like meets like
        mixed   indices, every problem at least once, with the codes dealt out so that every wavefront holds three or four
                different ones (problems of the rare codes more than once: see below); every problem of the families APART
                is the only one of them in its wavefront (its row moves with the wavefront's number), the other rows hold
                problems of the plain range
        alone   dict(index [4 P], active [4 P], slot [P]): problem i in row i % 4 of wavefront i (slot[i] = 4 i + i % 4),
                the other three rows not active and filled with a copy of the first `indef` problem
        tail    {count: the first `count` problems of sorted} for count in 1, 2, 3, 5"""
    rc_ref = np.asarray(rc_ref)
    family = np.asarray(family)
    P = int(n_problems)
    assert len(rc_ref) == P and len(family) == P
    srt = np.argsort(rc_ref, kind="stable")

    # mixed: the codes dealt round-robin.  A wavefront takes the next problem of the families APART, if one is left, into row
    # w % 4, and fills its other rows from the remaining problems class by class (class = the reference's code): always the
    # class with most problems not yet placed, no class a third time and only one class twice.  Three quarters of the
    # problems end with code 5, so the rare codes run out long before the common ones are placed: a class that has run
    # out starts again from its first problem, i.e. problems of rare codes meet several sets of neighbours.
    apart = [i for i in range(P) if family[i] in APART]
    klass = {}
    for i in range(P):
        if family[i] not in APART:
            klass.setdefault(int(rc_ref[i]), []).append(i)
    assert len(klass) >= 3
    taken = {c: 0 for c in klass}  # problems of the class handed out so far (beyond its size: again from the start)
    left = lambda c: max(len(klass[c]) - taken[c], 0)
    mixed, w = [], 0
    while apart or any(left(c) for c in klass):
        row, used = [None] * 4, {}
        if apart:
            row[w % 4] = apart.pop(0)
            used[int(rc_ref[row[w % 4]])] = 1
        for s in range(4):
            if row[s] is not None:
                continue
            doubled = any(v == 2 for v in used.values())
            allowed = [c for c in klass if used.get(c, 0) == 0 or (used[c] == 1 and not doubled and left(c) > 0)] or list(klass)
            c = max(allowed, key=lambda c: (left(c), -taken[c] / len(klass[c]), -c))
            row[s] = klass[c][taken[c] % len(klass[c])]
            taken[c] += 1
            used[c] = used.get(c, 0) + 1
        mixed += row
        w += 1
    mixed = np.array(mixed, dtype=np.int64)
    assert np.array_equal(np.unique(mixed), np.arange(P))

    garbage = int(np.nonzero(family == "indef")[0][0])
    slot = 4 * np.arange(P) + np.arange(P) % 4
    index = np.full(4 * P, garbage, dtype=np.int64)
    index[slot] = np.arange(P)
    active = np.zeros(4 * P, dtype=np.int32)
    active[slot] = 1
    return dict(sorted=srt, mixed=mixed, alone=dict(index=index, active=active, slot=slot), tail={c: srt[:c] for c in (1, 2, 3, 5)})


def check_product_golden(rc_got, x_got, clamp_got, n_free_got, g, i, n):
    """The product build (FMA contraction) on golden i of kernels.npz (g: the loaded file).  These goldens were picked to hit
    every exit and span 16 orders of magnitude in conditioning.  The exits -2 (search direction not a descent direction:
    sdotg >= 0), 2 (Armijo step below 1e-22) and 4 (relative improvement below 1e-8) are reached only when the quantity
    tested is at rounding resolution, so which one fires depends on the last bit (and -2 may turn into a regular exit); the
    FMA-free build reproduces them exactly."""
    t = tri(n)
    rc = int(g["qp_rc"][i])
    if rc == 1:  # 100 iterations on a numerically singular Hessian: how the crawl ends depends on the last bit
        assert rc_got in (-2, 1, 2, 4, 5), (i, rc, rc_got)
        return
    if rc in (-2, 2, 4):
        assert rc_got in (-2, 2, 4, 5), (i, rc, rc_got)
        if rc == -2 or rc_got == -2:
            return
    else:
        assert rc_got == rc, (i, rc)
        assert np.array_equal(clamp_got, g["qp_clamp"][i][:n]), (i, rc)
        assert n_free_got == g["qp_nfree"][i]
    if rc >= 1:
        H, gg = g["qp_H"][i][:t], g["qp_g"][i][:n]
        M = unpack(H, n)
        val = lambda x: float(x @ gg + 0.5 * x @ M @ x)
        vg, vr = val(x_got), val(g["qp_x"][i][:n])
        assert abs(vg - vr) <= 1e-7 * max(1.0, abs(vr)), (i, rc, vg, vr)
        assert np.all(x_got <= g["qp_hi"][i][:n]) and np.all(x_got >= g["qp_lo"][i][:n])
        if rc in (5, 6):
            scale = max(1.0, float(np.abs(g["qp_x"][i][:n]).max()))
            assert np.all(np.abs(x_got - g["qp_x"][i][:n]) <= 1e-7 * scale), (i, rc)
