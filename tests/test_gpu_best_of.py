"""Candidates per agent on the device: ilqg_batch_best_of / ilqg_batch_shift_winners, their _device forms and ilqg_multi_*.

A batch of B = G * K slots is G segments of K consecutive slots.  best_of is held to the numpy rule of tests/bestof_cases.py;
shift_winners to its composition through the host — x(), u(), that file's numpy statement, init(x0', u') — BIT FOR BIT in every
build: the kernels move data, the only arithmetic is the one fp64 add of du, so there is no tolerance to choose.
"""
import ctypes as C
import os

import numpy as np
import pytest

from bestof_cases import best_of_rule, shift_winners_rule
from oracle.harness import CAR_PARAMS, SYN_PARAMS_TIGHT, syn_inputs
from test_gpu_receding import assert_state_equal, setup, state

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ilqg():
    import __graft_entry__ as g
    g.load_package()
    from ddp_generator_amd import ilqg as m
    if not all(os.path.exists(m.library_path(p, fd, st)) for p, fd, st in
               (("carparking", 0, False), ("carparking", 0, "wave"), ("hxtest", 1, False), ("synth16x8", 1, False),
                ("synth10hx", 0, False), ("almix", 1, False))):
        g.build()
    if m.Problem("carparking", 0).device_count() < 1:
        pytest.fail("no HIP device visible: the GPU tests must run on the MI355X box")
    return m


def car(ilqg, B, N, strict=False, groups=0, first=40, **opts):
    from conftest import load_package
    x0, u0 = load_package().synth.car_batch(B, N, first=first)
    x0[B // 2:] *= 4.0   # (as test_gpu_receding.setup: a mix of steps accepted in the first and in the second stage)
    u0[B // 2:] *= 10.0
    return ilqg.BatchSolver("carparking", 0, batch=B, n_hor=N, params=CAR_PARAMS, opts=dict(opts, max_iter=40), strict=strict, groups=groups), x0, u0


def same_bits(a, b):
    """equal shapes, types and bits (-0.0 is not 0.0), every NaN equal to every other"""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    if a.dtype != np.float64:
        return bool(np.array_equal(a, b))
    nan = np.isnan(a)
    return bool(np.array_equal(nan, np.isnan(b)) and np.array_equal(a[~nan].view(np.int64), b[~nan].view(np.int64)))


def assert_same_bits(a, b, what):
    """assert_state_equal for states that hold NaN"""
    for k in a:
        assert same_bits(a[k], b[k]), "%s: %s differs" % (what, k)


def group_count(B, groups):
    """ilqg_batch_create_groups: whole tiles of 64 per group, no empty group"""
    per = -(-(-(-B // groups)) // 64) * 64
    return -(-B // per)


def launches(s):
    return {k: n for k, (n, _) in s.kernel_times().items() if n}


def compose(host, K, winner, steps, x0_new=None, u_tail=None, du=None):
    """the interval through the host: x(), u(), the numpy statement, init"""
    x0, u = shift_winners_rule(host.x(), host.u(), K, winner, steps, x0_new, u_tail, du)
    host.init(x0, u)


def on_device(arrays):
    import torch
    return [None if a is None else torch.tensor(np.ascontiguousarray(a), device="cuda:0") for a in arrays]


def shift_args(rng, B, K, N, nx, nu, steps, form, with_du, xh, winner):
    """x0_new [G, nx], u_tail [G, steps, nu], du [B, N, nu] of one argument form; du leaves each segment's winner (or its first
    slot) unperturbed"""
    G = B // K
    x0_new = rng.standard_normal((G, nx)) * 0.01 + xh[np.arange(G) * K, steps] if form != "neither" else None
    u_tail = 0.4 * rng.standard_normal((G, steps, nu)) if form == "both" else None
    du = None
    if with_du:
        du = 0.05 * rng.standard_normal((B, N, nu))
        du[np.where(np.asarray(winner) >= 0, winner, np.arange(G) * K)] = 0.0
    return x0_new, u_tail, du


# ---------------------------------------------------------------------------
# 1. best_of against the numpy rule
# ---------------------------------------------------------------------------
def fabricate(rng, B, K, turn):
    """scores and statuses with, segment by segment in turn: an exact tie of the two smallest, NaN and both infinities, status 7
    only, the winner in the first slot, in the last slot, NaN only, -0.0 against 0.0, nothing special; slots 31 and 32 of every
    64 tie below everything around them (one segment for K = 64, two neighbours else)"""
    score, status = rng.standard_normal(B), np.zeros(B, dtype=np.int32)
    status[rng.random(B) < 0.1] = 6
    status[rng.random(B) < 0.05] = 7
    for g in range(B // K):
        sl, kind = slice(g * K, g * K + K), (g + turn) % 8
        if kind == 0 and K > 1:
            status[sl] = 0
            score[g * K + K - 1] = score[g * K + K // 2] = score[sl].min() - 1.0
        elif kind == 1:
            score[g * K], score[g * K + K - 1], score[g * K + K // 2] = np.nan, np.inf, -np.inf
        elif kind == 2:
            status[sl] = 7
        elif kind == 3:
            score[g * K], status[g * K] = -100.0, 0
        elif kind == 4:
            score[g * K + K - 1], status[g * K + K - 1] = -100.0, 6
        elif kind == 5:
            score[sl] = np.nan
        elif kind == 6 and K > 1:
            score[sl], status[sl] = np.abs(score[sl]) + 1.0, 0
            score[g * K], score[g * K + K - 1] = 0.0, -0.0
    for at in range(31, B - 1, 64):
        score[at] = score[at + 1] = -50.0
        status[at] = status[at + 1] = 0
    return score, status


@pytest.mark.parametrize("B,groups", [(192, 1), (192, 2), (192, 4), (200, 1), (200, 2), (200, 4)])
def test_best_of_follows_the_numpy_rule(ilqg, B, groups):
    N = 20
    s, x0, u0 = car(ilqg, B, N, groups=groups)
    n_groups = s.groups()
    assert n_groups == group_count(B, groups)
    s.init(x0, u0)
    s.iterate(2)
    rng = np.random.default_rng(11)
    import torch  # (behind the first solver: one HIP runtime for both, see ilqg._share_hip_runtime)
    for K in (1, 2, 4, 8, 64):
        if B % K:
            continue
        for turn in range(8 if K >= 8 else 2):
            cost, status = fabricate(rng, B, K, turn)
            own, _ = fabricate(rng, B, K, turn + 3)
            s.set_scalar("cost", cost)
            s.set_ints("status", status)
            before = dict(state(s), gains=s.gains()[1])
            for score, ref in ((None, cost), (own, own)):
                want = best_of_rule(ref, status, K)
                s.timing(True)
                got = s.best_of(K, score)
                seen = launches(s)
                assert seen == {"k_best_of": n_groups}, seen
                dev_score = None if score is None else torch.tensor(score, device="cuda:0")
                got_dev = s.best_of(K, dev_score, device=True)
                torch.cuda.synchronize()
                assert launches(s) == {"k_best_of": 2 * n_groups}
                s.timing(False)
                for name, w, h, d in zip(("winner", "best", "n_eligible"), want, got, got_dev):
                    assert same_bits(w, h), "B=%d K=%d turn %d: %s of the host form" % (B, K, turn, name)
                    assert same_bits(w, d.cpu().numpy()), "B=%d K=%d turn %d: %s of the device form" % (B, K, turn, name)
            if turn == 0:
                assert_same_bits(dict(state(s), gains=s.gains()[1]), before, "the batch behind best_of")
    # only the winner is asked for
    w = np.zeros(B // 8, dtype=np.int32)
    s._ck(s.lib.ilqg_batch_best_of(s.h, 8, None, w.ctypes.data_as(C.c_void_p), None, None))
    assert np.array_equal(w, best_of_rule(cost, status, 8)[0])
    s.close()


# ---------------------------------------------------------------------------
# 2. shift_winners equals its composition through the host
# ---------------------------------------------------------------------------
def winners_for(name, dev, K, acc, idx, turn):
    """best_of's winners with a few set by hand: one segment at -1, the winner in slot gK and in slot gK + K - 1, and (lane
    mapping with kept roll-outs) in a segment whose members live in both locations the winner in X / U among losers in planes
    (even turns) or in a plane among losers in X / U (odd turns)"""
    winner = dev.best_of(K)[0].copy()
    G = winner.size
    winner[1], winner[2], winner[3] = -1, 2 * K, 3 * K + K - 1
    if name == "carparking":
        plane = ((acc == 1) & (idx <= 4)).reshape(G, K)  # (test_gpu_receding: where the current trajectory lives)
        mixed = [g for g in range(4, G) if plane[g].any() and not plane[g].all()]
        assert mixed, "no segment with members in both locations: %s of %d in planes" % (plane.sum(axis=1), K)
        g = mixed[0]
        winner[g] = g * K + int(np.flatnonzero(plane[g] if turn % 2 else ~plane[g])[0])
    return winner


@pytest.mark.parametrize("name,groups", [("carparking", 0), ("carparking", 2), ("carparking_wave", 0), ("hxtest", 0),
                                         ("synth16x8", 0), ("synth10hx", 0), ("almix", 0)])
def test_shift_winners_equals_the_host_composition(ilqg, name, groups):
    """Two batches with the same history (init, 7 iterations, as test_shift_equals_the_host_composition).  One is shifted by
    shift_winners — host arrays and CUDA tensors in turn —, the other through the host.  B = 200, K = 8; steps in {0, 1, 5,
    N - 1}; x0 / u_tail in the forms of the existing shift test, each with and without du."""
    B, K = 200, 8
    problem, fd, strict, N, params, opts, x0, u0 = setup(name, B)
    rng = np.random.default_rng(6)
    kw = dict(batch=B, n_hor=N, params=params, opts=dict(opts, max_iter=40), strict=strict, groups=groups)
    dev, host = ilqg.BatchSolver(problem, fd, **kw), ilqg.BatchSolver(problem, fd, **kw)
    if groups:
        assert dev.groups() == groups
    nx, nu = dev.problem.nx, dev.problem.nu
    turn = 0
    for form in ("both", "x0", "neither"):
        for with_du in (False, True):
            for s in (0, 1, 5, N - 1):
                for b in (dev, host):
                    b.init(x0, u0)
                    b.iterate(7)
                acc, idx = dev.ints("accepted"), dev.ints("alpha_idx")
                if name == "carparking":  # both locations occur (see test_shift_equals_the_host_composition)
                    assert np.any((acc == 1) & (idx <= 4)) and np.any((acc == 0) | (idx > 4))
                winner = winners_for(name, dev, K, acc, idx, turn // 2)
                xh = host.x()
                x0_new, u_tail, du = shift_args(rng, B, K, N, nx, nu, s, form, with_du, xh, winner)
                what = "%s %s du=%d s=%d" % (name, form, with_du, s)
                turn += 1
                if turn % 2:
                    dev.shift_winners(K, winner, s, x0_new, u_tail, du)
                else:
                    dev.shift_winners(K, *on_device([winner]), s, *on_device([x0_new, u_tail, du]))
                compose(host, K, winner, s, x0_new, u_tail, du)
                a, b = state(dev), state(host)
                assert_state_equal(a, b, what + " after the shift")
                assert np.all(a["iterations"] == 0) and np.all((a["status"] == 0) | (a["status"] == 7))
                dev.iterate(5)
                host.iterate(5)
                assert_state_equal(state(dev), state(host), what + " five iterations on")
    dev.close()
    host.close()


# ---------------------------------------------------------------------------
# 3. kernel boundaries
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("name,N", [("carparking", 6), ("carparking", 64), ("carparking", 65), ("carparking", 130),
                                    ("carparking_wave", 6), ("carparking_wave", 64), ("carparking_wave", 65), ("carparking_wave", 130),
                                    ("synth16x8", 31), ("synth16x8", 32), ("synth16x8", 33)])
def test_shift_winners_at_the_kernels_boundaries(ilqg, name, N):
    """n_hor = 6, 64, 65, 130: one, exactly one, one plus one and three rounds of k_shift_winners_lane's 64 steps (and one to three
    blocks of the wave form's 128 steps); synth16x8 (N_U = 8) at 31, 32, 33: the wave form's block of 256 / N_U = 32 steps.
    B = 72 with K = 4 (a tail tile of 8) and B = 128 with K = 64; steps in {1, n_hor - 1}; against the composition."""
    rng = np.random.default_rng(N)
    for B, K in ((72, 4), (128, 64)):
        if name == "synth16x8":
            x0, u0 = syn_inputs(B, N)
            kw = dict(batch=B, n_hor=N, params=SYN_PARAMS_TIGHT, opts=dict(max_iter=40))
            dev, host = ilqg.BatchSolver("synth16x8", 1, **kw), ilqg.BatchSolver("synth16x8", 1, **kw)
        else:
            strict = "wave" if name == "carparking_wave" else False
            (dev, x0, u0), (host, _, _) = car(ilqg, B, N, strict), car(ilqg, B, N, strict)
        nx, nu = dev.problem.nx, dev.problem.nu
        for s, form, with_du in ((1, "both", True), (N - 1, "both", True), (N - 1, "neither", False)):
            for b in (dev, host):
                b.init(x0, u0)
                b.iterate(3)
            winner = dev.best_of(K)[0].copy()
            winner[0] = -1
            winner[-1] = B - 1  # the last slot of the last tile
            x0_new, u_tail, du = shift_args(rng, B, K, N, nx, nu, s, form, with_du, host.x(), winner)
            dev.shift_winners(K, winner, s, x0_new, u_tail, du)
            compose(host, K, winner, s, x0_new, u_tail, du)
            assert_state_equal(state(dev), state(host), "%s N=%d B=%d K=%d s=%d %s" % (name, N, B, K, s, form))
            dev.iterate(2)
            host.iterate(2)
            assert_state_equal(state(dev), state(host), "%s N=%d B=%d K=%d s=%d %s two iterations on" % (name, N, B, K, s, form))
        dev.close()
        host.close()


# ---------------------------------------------------------------------------
# 4. identities
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["carparking", "carparking_wave"])
def test_own_winners_are_the_plain_shift(ilqg, name):
    """K = 1 with winner = arange(B), and K = 8 with every winner -1 (x0_new / u_tail repeated per slot for shift), equal shift()
    bit for bit in all three argument forms"""
    B, s = 200, 5
    problem, fd, strict, N, params, opts, x0, u0 = setup(name, B)
    kw = dict(batch=B, n_hor=N, params=params, opts=dict(opts, max_iter=40), strict=strict)
    plain, cand = ilqg.BatchSolver(problem, fd, **kw), ilqg.BatchSolver(problem, fd, **kw)
    rng = np.random.default_rng(9)
    for K, winner in ((1, np.arange(B)), (8, np.full(B // 8, -1))):
        for form in ("both", "x0", "neither"):
            for b in (plain, cand):
                b.init(x0, u0)
                b.iterate(7)
            G = B // K
            x0_new = rng.standard_normal((G, 4)) if form != "neither" else None
            u_tail = 0.4 * rng.standard_normal((G, s, 2)) if form == "both" else None
            plain.shift(s, None if x0_new is None else np.repeat(x0_new, K, axis=0), None if u_tail is None else np.repeat(u_tail, K, axis=0))
            cand.shift_winners(K, winner, s, x0_new, u_tail)
            assert_state_equal(state(cand), state(plain), "%s K=%d %s" % (name, K, form))
            plain.iterate(3)
            cand.iterate(3)
            assert_state_equal(state(cand), state(plain), "%s K=%d %s three iterations on" % (name, K, form))
    plain.close()
    cand.close()


@pytest.mark.parametrize("name", ["carparking", "carparking_wave"])
def test_reversed_segments_give_the_reversed_result(ilqg, name):
    B, K, s = 200, 8, 3
    problem, fd, strict, N, params, opts, x0, u0 = setup(name, B)
    kw = dict(batch=B, n_hor=N, params=params, opts=dict(opts, max_iter=40), strict=strict)
    fwd, rev = ilqg.BatchSolver(problem, fd, **kw), ilqg.BatchSolver(problem, fd, **kw)
    perm = (np.arange(B).reshape(-1, K)[:, ::-1]).reshape(-1)  # slot b of `rev` is slot perm[b] of `fwd`
    fwd.init(x0, u0)
    rev.init(x0[perm], u0[perm])
    fwd.iterate(7)
    rev.iterate(7)
    wf, bf, nf = fwd.best_of(K)
    wr, br, nr = rev.best_of(K)
    assert np.all(wf >= 0) and np.array_equal(perm[wr], wf) and np.array_equal(bf, br) and np.array_equal(nf, nr)
    du = 0.05 * np.random.default_rng(4).standard_normal((B, N, 2))
    fwd.shift_winners(K, wf, s, du=du)
    rev.shift_winners(K, wr, s, du=du[perm])
    a, b = state(fwd), state(rev)
    assert_state_equal(a, {k: v[perm] for k, v in b.items()}, "reversed segments")
    fwd.close()
    rev.close()


def test_groups_and_shards_give_the_single_batchs_bits(ilqg):
    """1 / 2 / 4 groups and two loop-back shards of 100 (a multiple of K = 4): winners and the shifted batch equal the single one's"""
    B, K, N, s = 200, 4, 500, 3
    rng = np.random.default_rng(8)
    G = B // K
    x0_new, u_tail, du = rng.standard_normal((G, 4)), 0.4 * rng.standard_normal((G, s, 2)), 0.05 * rng.standard_normal((B, N, 2))
    ref = None
    for groups in (1, 2, 4, "shards"):
        if groups == "shards":
            from conftest import load_package
            x0, u0 = load_package().synth.car_batch(B, N, first=40)
            x0[B // 2:] *= 4.0
            u0[B // 2:] *= 10.0
            b = ilqg.MultiSolver("carparking", 0, batch=B, n_hor=N, devices=[0] * 2, params=CAR_PARAMS, opts=dict(max_iter=40))
            cost, ints = b.costs, b.ints
        else:
            b, x0, u0 = car(ilqg, B, N, groups=groups)
            assert b.groups() == groups
            cost, ints = (lambda: b.scalar("cost")), b.ints
        b.init(x0, u0)
        b.iterate(4)
        out = list(b.best_of(K))
        score = np.cos(np.arange(B) * 0.7)
        out += list(b.best_of(K, score))
        assert np.array_equal(out[3], best_of_rule(score, ints("status"), K)[0])
        b.shift_winners(K, out[0], s, x0_new, u_tail, du)
        out += [b.x(), b.u(), cost(), ints("status"), ints("iterations")]
        b.iterate(3)
        out += [b.x(), b.u(), cost()]
        if ref is None:
            ref = out
        for i, (r, o) in enumerate(zip(ref, out)):
            assert np.array_equal(r, o), "%s: result %d differs from the single group's" % (groups, i)
        b.close()


# ---------------------------------------------------------------------------
# 5. failure stays local
# ---------------------------------------------------------------------------
def test_failure_stays_in_the_segment_that_received_it(ilqg):
    B, K, N, s = 64, 8, 40, 2
    (dev, x0, u0), (host, _, _) = car(ilqg, B, N), car(ilqg, B, N)
    for case in ("du", "x"):
        for b in (dev, host):
            b.init(x0, u0)
            b.iterate(3)
        winner = dev.best_of(K)[0].copy()
        du = np.zeros((B, N, 2))
        if case == "du":
            du[13] = np.nan  # one slot of segment 1
            hit = np.arange(B) == 13
        else:
            winner[2] = 2 * K + 5  # its x[steps] becomes x0 of all of segment 2
            for b in (dev, host):
                x = b.x()
                x[2 * K + 5, s] = np.nan
                b.set_x(x)
            hit = np.arange(B) // K == 2
        dev.shift_winners(K, winner, s, du=du)
        compose(host, K, winner, s, du=du)
        a = state(dev)
        assert_same_bits(a, state(host), "a NaN in " + case)
        print("NaN in %s: status 7 in slots %s" % (case, np.flatnonzero(a["status"] == 7)))
        assert np.array_equal(a["status"] == 7, hit), "status 7 in %s, expected in %s" % (np.flatnonzero(a["status"] == 7), np.flatnonzero(hit))
        assert np.all(a["status"][~hit] == 0)
    dev.close()
    host.close()


# ---------------------------------------------------------------------------
# 6. end to end
# ---------------------------------------------------------------------------
def test_three_intervals_equal_the_loop_through_the_host(ilqg):
    """{iterate(3); best_of; shift_winners(steps = 1, du)} three times, CarParking FULL_DDP 0, 25 agents x 8 candidates"""
    B, K, N = 200, 8, 500
    (dev, x0, u0), (host, _, _) = car(ilqg, B, N), car(ilqg, B, N)
    rng = np.random.default_rng(12)
    dev.init(x0, u0)
    host.init(x0, u0)
    for interval in range(3):
        dev.iterate(3)
        host.iterate(3)
        winner, best, n = dev.best_of(K)
        cost, status = host.scalar("cost"), host.ints("status")
        for got, want in zip((winner, best, n), best_of_rule(cost, status, K)):
            assert same_bits(got, want)
        # a sanity check that follows from the rule, no numeric claim: the winner is never worse than the segment's slot 0
        first = np.arange(B // K) * K
        ok = (winner >= 0) & np.isfinite(cost[first]) & (status[first] != 7)
        assert np.all(best[ok] <= cost[first][ok])
        du = 0.05 * rng.standard_normal((B, N, 2))
        du[winner[winner >= 0]] = 0.0
        dev.shift_winners(K, winner, 1, du=du)
        compose(host, K, winner, 1, du=du)
        assert_state_equal(state(dev), state(host), "interval %d" % interval)
    dev.close()
    host.close()


# ---------------------------------------------------------------------------
# 7. refusals
# ---------------------------------------------------------------------------
def test_refusals_leave_the_batch_untouched_and_name_the_argument(ilqg):
    B, K, N = 200, 8, 30
    s, x0, u0 = car(ilqg, B, N)
    import torch  # (behind the first solver: one HIP runtime for both, see ilqg._share_hip_runtime)
    s.init(x0, u0)
    s.iterate(2)
    before = state(s)
    lib, h, G = s.lib, s.h, B // K
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    w, best, n = np.zeros(B, dtype=np.int32), np.zeros(B), np.zeros(B, dtype=np.int32)
    good = s.best_of(K)[0]
    outside = good.copy()
    outside[3] = 4 * K  # the first slot of the next segment
    dw = torch.tensor(good, device="cuda:0")
    s.timing(True)
    calls = []
    for bad in (0, 3, 128, -8):  # the library's own refusals, past ilqg.py's
        calls += [(lambda bad=bad: lib.ilqg_batch_best_of(h, bad, None, p(w), p(best), p(n)), ("K = %d" % bad, "1, 2, 4, 8, 16, 32, 64")),
                  (lambda bad=bad: lib.ilqg_batch_shift_winners(h, bad, p(w), 1, None, None, None), ("K = %d" % bad, "1, 2, 4, 8, 16, 32, 64")),
                  (lambda bad=bad: lib.ilqg_batch_best_of_device(h, bad, None, C.c_void_p(dw.data_ptr()), None, None, None), ("K = %d" % bad,))]
    calls += [(lambda: lib.ilqg_batch_best_of(h, 16, None, p(w), None, None), ("K = 16", "B % K")),
              (lambda: lib.ilqg_batch_shift_winners(h, 16, p(w), 1, None, None, None), ("K = 16", "B % K")),
              (lambda: lib.ilqg_batch_best_of(h, K, None, None, p(best), p(n)), ("winner is NULL",)),
              (lambda: lib.ilqg_batch_shift_winners(h, K, None, 1, None, None, None), ("winner is NULL",)),
              (lambda: lib.ilqg_batch_shift_winners_device(h, K, None, 1, None, None, None, None), ("winner is NULL",)),
              (lambda: lib.ilqg_batch_shift_winners(h, K, p(outside), 1, None, None, None), ("winner[3] = 32", "outside segment 3")),
              (lambda: lib.ilqg_batch_best_of_device(h, K, None, p(w), None, None, None), ("winner", "device memory")),
              (lambda: lib.ilqg_batch_best_of_device(h, K, p(best), C.c_void_p(dw.data_ptr()), None, None, None), ("score", "device memory")),
              (lambda: lib.ilqg_batch_shift_winners_device(h, K, p(good), 1, None, None, None, None), ("winner", "device memory")),
              (lambda: lib.ilqg_batch_shift_winners_device(h, K, C.c_void_p(dw.data_ptr()), 1, None, None, p(np.zeros((B, N, 2))), None),
               ("du", "device memory"))]
    for steps in (-1, N, N + 1):
        calls += [(lambda steps=steps: lib.ilqg_batch_shift_winners(h, K, p(good), steps, None, None, None), ("steps = %d" % steps, "n_hor")),
                  (lambda steps=steps: lib.ilqg_batch_shift_winners_device(h, K, C.c_void_p(dw.data_ptr()), steps, None, None, None, None),
                   ("steps = %d" % steps, "n_hor"))]
    for call, words in calls:
        assert call() != 0
        msg = lib.ilqg_batch_error(h).decode()
        assert all(x in msg for x in words), msg
    for call, words in ((lambda: s.best_of(3), ("K",)), (lambda: s.shift_winners(K, outside, 1), ("winner[3]", "outside segment")),
                        (lambda: s.shift_winners(K, good, N), ("steps",))):
        with pytest.raises(ilqg.IlqgError) as e:
            call()
        assert all(x in str(e.value) for x in words), str(e.value)
    assert launches(s) == {}
    s.timing(False)
    assert_state_equal(state(s), before, "refused calls")
    s.close()
    # a shard boundary that cuts a segment: two shards of 100, K = 8
    m = ilqg.MultiSolver("carparking", 0, batch=B, n_hor=N, devices=[0] * 2, params=CAR_PARAMS, opts=dict(max_iter=40))
    m.init(x0, u0)
    xm, um = m.x(), m.u()
    for call in (lambda: m.best_of(K), lambda: m.shift_winners(K, good, 1)):
        with pytest.raises(ilqg.IlqgError) as e:
            call()
        assert "K = 8" in str(e.value) and "not a multiple of K" in str(e.value) and "segment" in str(e.value)
    other = np.full(B // 4, -1, dtype=np.int32)
    other[25] = 99  # segment 25 is the second shard's first; slot 99 belongs to the first shard
    with pytest.raises(ilqg.IlqgError) as e:
        m.shift_winners(4, other, 1)
    assert "winner[25] = 99" in str(e.value) and "outside segment 25" in str(e.value)
    assert np.array_equal(m.x(), xm) and np.array_equal(m.u(), um)
    m.close()
