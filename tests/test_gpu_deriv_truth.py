"""The device's derivative records against the derivatives of the problem's DEFINITION (tests/golden/deriv_truth.npz: the
points, parameters, multipliers, weights and the truth tests/deriv_cases.py computed in 80-digit arithmetic; read here with
numpy alone), per entry and normalised by the size of the entry's own array at its step — not by max(1, |ref|), under which
an entry of size 1e-6 is held to four digits.

calc_derivs() + derivs() of a batch of 70 (one full wavefront and a tail): every even trajectory is the case, every odd one
the case with its steps in reverse order (problems with a per-time-step parameter: repeated only, but for the rows twin under
a window per trajectory, which is reversed along with the steps).  Kernels: k_derivs in product and FMA-free builds, its rows
twin under a nominal per-trajectory table and a per-trajectory window, k_derivs_wave<false> on the n = 16 and n = 10 libraries.

THE BAR of a library is a ratio to the reference build's stored error for the same problem (never to the device's own
output): the next power of two above the worst ratio measured on an MI355X, profiles/r22_deriv_truth.txt.  FMA contraction
and the device's 2-ulp sincos make a ratio of a few expected; above 64 would be a finding, not a bar.  Measured, worst per
group of libraries (every single one in the profile):
    k_derivs, product and FMA-free builds (carparking 0/1, hxtest 0/1, almix 0/1, brachi 1, brachi_hli 0/1)      1.00
    its rows twins (carparking 1, hxtest 1 under a table; almix 1, brachi_hli 1 under table and window)           1.00
    k_derivs_wave<false>: synth16x8 0 1.00, synth16x8 1 / synth16x8_plain 1 0.88, synth16p 1 0.82,
                          synth10hx 0 1.12, synth10hx 1 1.31; FMA-free builds 1.00, synth10hx 1 1.31              1.31
so every bar is 2.
The FMA-free build of AlMix (only + - * / sqrt) gives the CPU restatement's record bit for bit.

Not reachable here: the factored records of k_derivs_wave<true> and of k_derivs_parts are transient (the shim hands records
that a caller reads to k_derivs_wave<false>, whole), and the fused sweep's derivatives have no getter; they stay held through
the gains they produce (tests/test_gpu_parity.py).  The generated forms those kernels call are held to the same truth on the
host (tests/test_deriv_forms.py)."""
import numpy as np
import pytest

import deriv_cases as DC
from conftest import golden
from oracle.harness import Driver, lib_path

pytestmark = pytest.mark.gpu

B = 70
# (library group -> bar on device error / reference-build error: the next power of two above the worst ratio measured)
RATIO_BAR = dict(lane=2.0, lane_strict=2.0, rows=2.0, rows_strict=2.0, wave=2.0, wave_strict=2.0)

PER_STEP = {"almix": "vref", "brachi_hli": "ymin"}

# (case, library, FULL_DDP, strict, mode): mode "" plain, "params" nominal per-trajectory table, "steps" that and a window
LANE = [("carparking", "carparking", 0), ("carparking", "carparking", 1), ("hxtest", "hxtest", 0), ("hxtest", "hxtest", 1),
        ("almix", "almix", 0), ("almix", "almix", 1), ("almix_b", "almix", 1), ("brachi", "brachi", 1), ("brachi_hli", "brachi_hli", 0),
        ("brachi_hli", "brachi_hli", 1)]
WAVE = [("synth10hx", "synth10hx", 0), ("synth10hx", "synth10hx", 1), ("synth16x8", "synth16x8", 0), ("synth16x8", "synth16x8", 1),
        ("synth16p", "synth16p", 1)]
LIBS = ([c + (strict, "") for c in LANE for strict in (False, True)]
        + [c + (strict, "") for c in WAVE for strict in (False, True)] + [("synth16x8", "synth16x8_plain", 1, False, "")]
        + [("carparking", "carparking", 1, strict, "params") for strict in (False, True)]
        + [("hxtest", "hxtest", 1, False, "params")]
        + [("almix", "almix", 1, strict, "steps") for strict in (False, True)]
        + [("brachi_hli", "brachi_hli", 1, False, "steps")])


@pytest.fixture(scope="module")
def ilqg():
    import __graft_entry__ as g
    g.build_for_tests()
    from ddp_generator_amd import ilqg as m
    if m.Problem("carparking", 0).device_count() < 1:
        pytest.fail("no HIP device visible: the GPU tests must run on the MI355X box")
    return m


def group_of(problem, strict, mode, wave):
    return ("wave" if wave else "rows" if mode else "lane") + ("_strict" if strict else "")


def case_of(g, name):
    pre = name + "/"
    params = {k[len(pre) + 6:]: g[k] for k in g.files if k.startswith(pre + "param/")}
    return dict(params=params, xs=g[pre + "xs"], us=g[pre + "us"], el=g[pre + "el_struct"], fin_mul=g[pre + "fin_struct"],
                w_pen=g[pre + "w_pen"], steps=g[pre + "steps"].astype(int), rec=g[pre + "rec"], fin=g[pre + "fin"])


def device_records(ilqg, c, library, fd, strict, mode, reverse):
    N = DC.N_HOR
    xs, us, el = c["xs"], c["us"], c["el"]
    rev = np.arange(N)[::-1]
    x = np.repeat(xs[None], B, axis=0)
    u = np.repeat(us[None], B, axis=0)
    run = np.repeat(el[None], B, axis=0)
    if reverse:
        x[1::2, :N] = xs[rev]
        u[1::2] = us[rev]
        run[1::2] = el[rev]
    has_mul = bool(el.shape[1] or len(c["fin_mul"]))
    # (the derivative kernels take the penalty weights of the last accepted step, which init() sets from the options)
    opts = dict(w_pen_init_l=float(c["w_pen"][0]), w_pen_init_f=float(c["w_pen"][1])) if has_mul else {}
    s = ilqg.BatchSolver(library, fd, batch=B, n_hor=N, params=c["params"], opts=opts, strict=strict)
    s.init(x[:, 0], u)
    if mode:  # the rows twins: every trajectory its own row of the nominal values (and its own window)
        per_step = PER_STEP.get(library)
        s.set_params_batch({k: np.repeat(np.atleast_2d(v), B, axis=0) for k, v in c["params"].items() if k != per_step})
        if mode == "steps":
            w = np.repeat(np.asarray(c["params"][per_step])[None], B, axis=0)
            if reverse:
                w[1::2, :N] = w[1::2, :N][:, rev]
            s.set_param_steps_batch(per_step, w)
    s.set_x(x)
    s.set_u(u)
    assert has_mul == bool(sum(s.multiplier_dims()))
    if has_mul:
        s.set_multipliers(run, np.repeat(c["fin_mul"][None], B, axis=0))
    s.set_ints("need_derivs", 1)
    s.calc_derivs()
    rec, fin = s.derivs()
    facts = dict(nd=s.problem.rec_dev, wave=s.problem.wave_mapping, n=s.problem.nx, m=s.problem.nu)
    assert np.all(s.ints("status") == 0)
    s.close()
    return rec, fin, facts


@pytest.mark.parametrize("name,library,fd,strict,mode", LIBS)
def test_device_records_equal_derivatives_of_the_definition(ilqg, oracle_built, name, library, fd, strict, mode):
    g = golden("deriv_truth.npz")
    c = case_of(g, name)
    ref = float(g[DC.key_of(name, fd)])
    problem = library.replace("_plain", "")
    reverse = problem not in PER_STEP or mode == "steps"
    rec, fin, f = device_records(ilqg, c, library, fd, strict, mode, reverse)
    n, m, N = f["n"], f["m"], DC.N_HOR
    want = c["rec"] if fd else DC.drop_tensors(c["rec"], n, m)
    # the arrays the device record holds: its leading rec_dev entries (the limits' signs and gradients only where the limits
    # depend on the state)
    held, o = [], 0
    for arr, cnt in DC.segments(n, m, fd):
        o += cnt
        if o <= f["nd"]:
            held.append(arr)
    assert held[:9] == ["cx", "cxx", "cu", "cuu", "cxu", "fx", "fu", "lower", "upper"] and (not fd or "fxu" in held)
    worst = 0.0
    for b in range(B):
        at = (N - 1 - c["steps"]) if (reverse and b % 2) else c["steps"]
        worst = max(worst, DC.error(rec[b][at], want, n, m, fd, only=held), DC.error(fin[b], c["fin"], n, m, fd, final=True))
    group = group_of(problem, strict, mode, f["wave"])
    print("RATIO %s fd%d %s %s %s: device %.3g reference build %.3g ratio %.2f" % (library, fd, "strict" if strict else "product", mode or "-", group,
                                                                                 worst, ref, worst / ref))
    assert worst <= RATIO_BAR[group] * ref, (library, fd, strict, mode, worst, ref, worst / ref)

    if strict and problem == "almix":  # only + - * / sqrt: the FMA-free build gives the CPU restatement's bits
        d = Driver(lib_path("oracle", "almix", fd), N, c["params"], dict(max_iter=1))
        assert d.init(c["xs"][0], c["us"]) == 1
        d.set_multipliers(c["el"], c["fin_mul"])
        d.set_state(c["xs"], c["us"], 0.0, 1.0, tuple(c["w_pen"]))
        assert d.cost_resweep() == 1 and d.calc_derivs() == 1
        orec, ofin = d.derivs()
        d.close()
        for b in range(B):
            at = (N - 1 - np.arange(N)) if (reverse and b % 2) else np.arange(N)
            assert np.array_equal(rec[b][at][:, :f["nd"]], orec[:, :f["nd"]]) and np.array_equal(fin[b], ofin), b
