"""Every device form of the line search on each branch of line_search.c:37-75: the cases of tests/linesearch_cases.py
(pinned to the reference's own line_search() by tests/test_linesearch_cases_recipe.py, no GPU), one search per solver —
init, set_gains, the scalars cost / dV0 / dV1 and sentinels in dcost / expected, line_search(), the reads — and sequences of
four searches that move the current trajectories between X / U and the kept planes.

Compared on every trajectory: alpha_idx, accepted and alpha_ok of every rolled step size exactly, in every build;
alpha_cost of every finite rolled step size, new_cost, dcost, expected and the trajectory left behind (the reference's
candidate when accepted; when not, the nominal read before the search, bit for bit in every build) — bit for bit in the
FMA-free libraries, at the suite's single-pass bar (1e-10 relative to max(1, |ref|)) in the product libraries.  Left out:
alpha_cost of failed roll-outs and new_cost behind a failed last one (the reference returns a partial sum), dcost /
expected where nothing tried was finite (no reference value: the device keeps the sentinels, which is asserted), and the
exact z == zMin tie in the product builds."""
import numpy as np
import pytest

import linesearch_cases as LS

pytestmark = pytest.mark.gpu
TOL = 1e-10


@pytest.fixture(scope="module")
def ilqg():
    import __graft_entry__ as g
    g.build_for_tests()
    from ddp_generator_amd import ilqg as m
    if m.Problem("carparking", 0).device_count() < 1:
        pytest.fail("no HIP device visible: the GPU tests must run on the MI355X box")
    return m


def worst(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.max(np.abs(a - b) / np.maximum(1.0, np.abs(b)))) if a.size else 0.0


# ls_keep = 2 (the default): k_search while the first stage has at most 4 step sizes (PLANE_A).  ls_split 4, 3, 1: two stages
# over 8 step sizes; over 4, 2 and 1 step sizes ls_split = 4 is the search WITHOUT a second stage (k_rejected_home)
KEEP2 = (dict(ls_split=4), dict(ls_split=3), dict(ls_split=1))
# k_rollout + k_select: ls_keep 1 and 0, and ls_keep = 2 with a first stage of 8 step sizes, which the shim hands to them too.
# ls_split = 1: the scan state crosses a stage boundary in these forms on every batch, the one of 2 step sizes included
PLAIN = (dict(ls_keep=1, ls_split=0), dict(ls_keep=1, ls_split=3), dict(ls_keep=1, ls_split=1), dict(ls_keep=0, ls_split=3), dict(ls_keep=0, ls_split=1),
         dict(ls_split=8))
CAR_BATCHES = ["car6", "car2", "car3", "car6z", "car6a4", "car6a2", "car6a1"]
FIELDS = ("idx", "acc", "ok", "ac", "new_cost", "dcost", "expected", "x", "u", "x_before", "u_before")


def search(ilqg, name, build, opts, B=None, groups=0, rows=False):
    """one line search of the first B cases of batch `name` in library build `build` (False, True: FMA-free, "wave")"""
    r = LS.reference(name)
    problem, n, params, o = LS.setup(name)
    B = B or len(r["cls"])
    s = ilqg.BatchSolver(problem, 0, batch=B, n_hor=n, params=params, opts=dict(o, **opts), strict=build, groups=groups)
    if rows:  # a nominal per-trajectory table: the rows twins of the kernels
        s.set_params_batch({k: np.tile(np.asarray(params[k], dtype=np.float64), (B, 1)) for k in ("d", "h")})
    s.init(r["x0"][:B], r["u0"][:B])
    assert np.all(s.ints("status") == 0)
    s.set_gains(r["l"][:B], r["L"][:B])
    for k in ("cost", "dV0", "dV1"):
        s.set_scalar(k, r[k][:B])
    for k, v in LS.SENTINEL.items():
        s.set_scalar(k, v)
    before = s.x(), s.u()
    s.line_search()
    A = len(LS.BATCHES[name][2])
    out = dict(idx=s.ints("alpha_idx"), acc=s.ints("accepted"), ok=s.ints("alpha_ok")[:, :A], ac=s.scalar("alpha_cost")[:, :A],
               new_cost=s.scalar("new_cost"), dcost=s.scalar("dcost"), expected=s.scalar("expected"), x=s.x(), u=s.u(),
               x_before=before[0], u_before=before[1], groups=s.groups())
    s.close()
    return out


def held(name, out, exact, split, what):
    """the comparison of the module docstring; returns the worst deviation of the compared doubles"""
    r = LS.reference(name)
    A, B = len(LS.BATCHES[name][2]), len(out["idx"])
    s1 = split if 0 < split < A else A
    use = np.ones(B, dtype=bool) if exact else r["tie"][:B] == 0
    ref = {k: r[k][:B][use] for k in LS.FIELDS}
    got = {k: out[k][use] for k in FIELDS}
    assert np.array_equal(got["idx"], ref["idx"]) and np.array_equal(got["acc"], ref["ret"]), (what, got["idx"], ref["idx"])
    # rolled: the first stage's step sizes for everybody, the second's for the trajectories the first left undecided
    rolled = (np.arange(A)[None, :] < s1) | (ref["idx"][:, None] > s1)
    assert np.array_equal(got["ok"][rolled], ref["ok"][rolled]), what
    fin = rolled & (ref["ok"] == 1)
    rej = ref["ret"] == 0
    nc, de = ref["cmp_new_cost"] == 1, ref["cmp_dexp"] == 1
    pairs = [("alpha_cost", got["ac"][fin], ref["ac"][fin]), ("new_cost", got["new_cost"][nc], ref["new_cost"][nc]),
             ("dcost", got["dcost"][de], ref["dcost"][de]), ("expected", got["expected"][de], ref["expected"][de]),
             ("x", got["x"], ref["xc"]), ("u", got["u"], ref["uc"])]
    dev = {k: worst(a, b) for k, a, b in pairs}
    print("%s %s: worst deviation " % (name, what) + ", ".join("%s %.3g" % kv for kv in dev.items()))
    for k, a, b in pairs:
        assert np.array_equal(a, b) if exact else dev[k] <= TOL, (what, k, dev[k])
    # nothing tried was finite: the fields keep what they held; nothing accepted: the nominal comes back untouched
    assert np.all(got["dcost"][~de] == LS.SENTINEL["dcost"]) and np.all(got["expected"][~de] == LS.SENTINEL["expected"]), what
    assert np.array_equal(got["x"][rej], got["x_before"][rej]) and np.array_equal(got["u"][rej], got["u_before"][rej]), what
    return max(dev.values())


def same_bits(a, b, what):
    for k in FIELDS:
        assert np.array_equal(a[k], b[k], equal_nan=True), (what, k)


def no_dma(monkeypatch, off):
    if off:
        monkeypatch.setenv("ILQG_NO_DMA", "1")
    else:
        monkeypatch.delenv("ILQG_NO_DMA", raising=False)


@pytest.mark.parametrize("strict", [False, True])
@pytest.mark.parametrize("name", CAR_BATCHES)
def test_lane_mapping_forms(ilqg, monkeypatch, name, strict):
    """k_search in both stages, and alone where the list has no more step sizes than the first stage, with the records through
    LDS and per lane (KEEP2); k_rollout + k_select in one stage, with the second stage beside the winners (ls_keep = 1) and
    re-rolled (ls_keep = 0) (PLAIN)"""
    top = 0.0
    for opts in KEEP2:
        for off in (False, True):
            no_dma(monkeypatch, off)
            top = max(top, held(name, search(ilqg, name, strict, opts), strict, opts["ls_split"], "%s%s" % (opts, " per-lane loads" if off else "")))
    no_dma(monkeypatch, False)
    for opts in PLAIN:
        top = max(top, held(name, search(ilqg, name, strict, opts), strict, opts["ls_split"], str(opts)))
    print("%s strict=%s: worst deviation over the forms %.3g" % (name, strict, top))


@pytest.mark.parametrize("strict", [False, True])
def test_lane_mapping_batch_sizes_and_stream_groups(ilqg, monkeypatch, strict):
    """one trajectory; 37 (the last wavefront partly filled for T = 16 and T = 21 trajectories to a wavefront); the whole
    table as 1, 2 and 4 stream groups"""
    for opts in (dict(ls_split=4), dict(ls_split=3), dict(ls_keep=1, ls_split=3)):
        for off in (False, True) if "ls_keep" not in opts else (False,):
            no_dma(monkeypatch, off)
            for B in (1, 37):
                held("car6", search(ilqg, "car6", strict, opts, B=B), strict, opts["ls_split"], "%s B=%d" % (opts, B))
            for groups in (1, 2, 4):
                out = search(ilqg, "car6", strict, opts, groups=groups)
                assert out["groups"] == groups
                held("car6", out, strict, opts["ls_split"], "%s groups=%d" % (opts, groups))
    no_dma(monkeypatch, False)


@pytest.mark.parametrize("strict", [False, True])
@pytest.mark.parametrize("name", CAR_BATCHES)
def test_rows_twins(ilqg, monkeypatch, name, strict):
    """the kernels instantiated for per-trajectory parameters, under a table that repeats the shared values: held to the
    reference like the shared forms, and in the FMA-free build bit for bit the shared run"""
    for opts in KEEP2:
        for off in (False, True):
            no_dma(monkeypatch, off)
            out = search(ilqg, name, strict, opts, rows=True)
            held(name, out, strict, opts["ls_split"], "rows %s%s" % (opts, " per-lane loads" if off else ""))
            if strict:
                same_bits(out, search(ilqg, name, strict, opts), (name, opts, off))
    no_dma(monkeypatch, False)


@pytest.mark.parametrize("name", CAR_BATCHES)
def test_wave_mapping(ilqg, name):
    """CarParking forced into the wave mapping, default path: k_rollout_parts, k_select from the list, k_adopt, k_adopt_first"""
    held(name, search(ilqg, name, "wave", {}), False, 1, "wave mapping")
    held(name, search(ilqg, name, "wave", dict(ls_split=3)), False, 3, "wave mapping ls_split=3")


@pytest.mark.parametrize("strict", [False, True])
def test_brachi(ilqg, strict):
    """a problem with multipliers (the searches load them per step), default options"""
    held("brachi6", search(ilqg, "brachi6", strict, {}), strict, 4, "brachi")
    held("brachi6", search(ilqg, "brachi6", strict, dict(ls_split=1)), strict, 1, "brachi ls_split=1")


# ---------------------------------------------------------------------------
# sequences: where the current trajectory lives
# ---------------------------------------------------------------------------
def replay(ilqg, ref, strict, upto, iterate=False):
    """the first `upto` searches of an LS.sequence_reference on the device, WITHOUT a host read or write of a trajectory
    between them (either brings every trajectory home); then (alpha_idx [upto, B], accepted [upto, B], x, u).  iterate: the
    whole iteration in one call — the cost alone steers; else the stages, with the reference's dV set behind the backward
    pass (the device's own where the reference took the driver's own)"""
    from oracle.harness import CAR_PARAMS
    s = ilqg.BatchSolver("carparking", 0, batch=LS.SEQ_B, n_hor=ref["n_hor"], params=CAR_PARAMS, strict=strict,
                         opts=dict(alpha=ref["alpha"], zMin=ref["zMin"], fuse_derivs=0, max_iter=100))
    s.init(ref["x0"], ref["u0"])
    idx, acc = [], []
    for k in range(upto):
        s.set_option("ls_split", ref["splits"][k])
        s.set_scalar("lambda", ref["lam"])
        s.set_scalar("dlambda", 1.0)
        s.set_scalar("cost", ref["cost"][k])
        if iterate:
            s.iterate(1)
        else:
            s.calc_derivs()
            s.back_pass()
            if ref["steer"] == "dV":
                s.set_scalar("dV0", ref["dV"][k, :, 0])
                s.set_scalar("dV1", ref["dV"][k, :, 1])
            s.line_search()
            s.update()
        idx.append(s.ints("alpha_idx"))
        acc.append(s.ints("accepted"))
        assert np.all(s.ints("status") == 0), k
    out = np.array(idx), np.array(acc), s.x(), s.u()
    s.close()
    return out


def in_a_plane(ref, k, what):
    """the trajectories to which `what` happens in search k while they live in a plane: accepted in search k - 1's first stage"""
    return np.array([w == what and before == "first" for w, before in zip(ref["what"][k], ref["what"][k - 1])])


def follows_the_driver(ref, exact, upto, idx, acc, x, u, what):
    """indices and acceptances exactly; the nominal the search leaves bit for bit (exact) or at the single-pass bar"""
    assert np.array_equal(idx, ref["idx"][:upto]) and np.array_equal(acc, ref["ret"][:upto]), (what, upto)
    dx, du = worst(x, ref["x"][upto - 1]), worst(u, ref["u"][upto - 1])
    print("%s exact %s after search %d: x %.3g, u %.3g from the driver's" % (what, exact, upto, dx, du))
    if exact:
        assert np.array_equal(x, ref["x"][upto - 1]) and np.array_equal(u, ref["u"][upto - 1]), (what, upto)
    else:
        assert dx <= TOL and du <= TOL, (what, upto, dx, du)


def rejected_come_back_untouched(ref, seen):
    """what a search rejects is, bit for bit, what the search before left — in every build; also out of a plane"""
    for k in range(1, len(seen)):
        rej = ref["ret"][k] == 0
        assert rej.sum() >= 8
        assert np.array_equal(seen[k][0][rej], seen[k - 1][0][rej]) and np.array_equal(seen[k][1][rej], seen[k - 1][1][rej]), k


@pytest.mark.parametrize("strict", [False, True])
@pytest.mark.parametrize("n_alpha", [8, 4])
def test_sequences_of_searches(ilqg, oracle_built, n_alpha, strict):
    """the plan of LS.SEQ_PLAN with every index planned (dV steers): (a) accepted in the first stage, (b) rejected while living
    in a plane / accepted in the second stage / first, (c), (d) accepted in the second stage while living in a plane, (e) the
    other ls_split (all_home) — per trajectory mixed.  With 4 step sizes the first four searches have no second stage
    (k_rejected_home)."""
    ref = LS.sequence_reference(n_alpha, "dV")
    S = len(LS.SEQ_PLAN)
    if n_alpha == 8:
        assert all(in_a_plane(ref, k, "second").sum() >= 8 for k in (2, 3))
    assert in_a_plane(ref, 1, "reject").sum() >= 8
    seen = []
    for upto in range(1, S + 1):
        idx, acc, x, u = replay(ilqg, ref, strict, upto)
        follows_the_driver(ref, strict, upto, idx, acc, x, u, "dV-steered, %d step sizes, strict %s" % (n_alpha, strict))
        seen.append((x, u))
    rejected_come_back_untouched(ref, seen)


@pytest.mark.parametrize("strict", [False, True])
@pytest.mark.parametrize("n_alpha", [8, 2])
def test_iterate_commits_like_the_stages(ilqg, oracle_built, n_alpha, strict):
    """the commit folded into k_update (iterate) against k_commit (line_search + update): the same plan steered by the cost
    alone, under the backward pass's own dV.  With 8 step sizes (a first stage of 2) trajectories are accepted in the second
    stage and rejected while they live in a plane; with 2 step sizes the first four searches have no second stage
    (k_rejected_home).  iterate gives the stages' bits after every search, in every build, and both follow the driver: indices
    and acceptances exactly, the trajectories at 1e-10 relative to max(1, |ref|) in the FMA-free build too — the callbacks'
    sin / cos are the device's own straight-line routine, within 2 ulp of the host's (test_device_sincos_accuracy), so over
    100 steps and five iterations an FMA-free roll-out is the driver's only to the last places (seen: 4.4e-16 after the first
    search), unlike the 12-step sequences above, which are the driver's bit for bit."""
    ref = LS.sequence_reference(n_alpha, "cost")
    S = len(LS.SEQ_PLAN)
    if n_alpha == 8:
        moved = [int(in_a_plane(ref, k, "second").sum()) for k in range(1, S)]
        print("accepted in the second stage while living in a plane, per search:", moved)
        assert sum(m >= 3 for m in moved) >= 2, moved
    assert in_a_plane(ref, 1, "reject").sum() >= 8
    seen = []
    for upto in range(1, S + 1):
        staged, fused = replay(ilqg, ref, strict, upto), replay(ilqg, ref, strict, upto, iterate=True)
        for a, b in zip(staged, fused):
            assert np.array_equal(a, b), upto
        follows_the_driver(ref, False, upto, *staged, "cost-steered, %d step sizes, strict %s" % (n_alpha, strict))
        seen.append(staged[2:])
    rejected_come_back_untouched(ref, seen)
