"""The cases of tests/test_gpu_launch_plan.py: one small solve per branch of the device shim's launch layer of an iteration
(csrc/ilqg_shim_impl.inc: dev_fill, wave_backward, ilqg_dev_backward, ilqg_dev_search, launch_rollout), each with the launch
counts kernel_times() reports for it.  tests/golden/launch_counts_parent.json holds those counts as the commit BEFORE the
launch layer was restated gave them (profiles/r19_launch_layer.txt); a change to these functions that launches another
kernel, or one more or less often, fails the test.

Lane mapping: B = 73 (one full tile of 64 and a ragged one), n_hor = 6, one stream group and two.  Wave mapping: B = 9 (two
full quads of four trajectories and a ragged one), n_hor = 6."""
import numpy as np

from oracle.harness import SYN10_PARAMS, SYN_PARAMS_TIGHT, SYNP_PARAMS_TIGHT, syn10_inputs, syn_inputs

# the switches of the environment a case may set; every other one of them is unset while it runs
ENV = ("ILQG_NO_QUAD", "ILQG_QUAD_SPEC", "ILQG_QUAD_STORED", "ILQG_TWO_PIECES", "ILQG_DERIV_PARTS", "ILQG_NO_DMA", "ILQG_NO_ROLLOUT_PARTS",
       "ILQG_WORK_GB")
N = 6
ARRAYS = ("cost", "lambda", "dV0", "dV1", "g_norm")
INTS = ("status", "alpha_idx", "bp_calls")


def case(name, problem, fd, build=False, B=9, n_hor=N, groups=0, opts=None, env=None, staged=False, table=False):
    return dict(name=name, problem=problem, fd=fd, build=build, B=B, n_hor=n_hor, groups=groups, opts=opts or {}, env=env or {}, staged=staged,
                table=table)


def lane(name, problem="carparking", fd=0, **kw):
    return [case("%s_g%d" % (name, g), problem, fd, B=73, groups=g, **kw) for g in (1, 2)]


CASES = (
    lane("car_keep2_split4", opts=dict(ls_keep=2, ls_split=4)) + lane("car_keep2_split0", opts=dict(ls_keep=2, ls_split=0)) +
    lane("car_keep1_split4", opts=dict(ls_keep=1, ls_split=4)) + lane("car_keep0_split4", opts=dict(ls_keep=0, ls_split=4)) +
    lane("car_keep0_split0", opts=dict(ls_keep=0, ls_split=0)) + lane("car_unfused", opts=dict(fuse_derivs=0)) +
    lane("car_no_dma", opts=dict(ls_keep=2), env=dict(ILQG_NO_DMA="1")) + lane("car_rows", table=True) + lane("car_staged", staged=True) +
    lane("almix_fd1", "almix", 1) + [
        case("syn_fd1", "synth16x8", 1),
        case("syn_fd1_no_spec", "synth16x8", 1, env=dict(ILQG_QUAD_SPEC="0")),
        case("syn_fd1_no_quad", "synth16x8", 1, env=dict(ILQG_NO_QUAD="1")),
        case("syn_fd1_two_pieces", "synth16x8", 1, env=dict(ILQG_TWO_PIECES="1")),
        case("syn_fd1_unfused", "synth16x8", 1, opts=dict(fuse_derivs=0)),
        case("syn_fd1_no_rollout_parts", "synth16x8", 1, env=dict(ILQG_NO_ROLLOUT_PARTS="1")),
        case("syn_fd1_no_dma", "synth16x8", 1, env=dict(ILQG_NO_DMA="1")),
        # the smallest work buffer the shim makes (one trajectory of complete records): the factored records of 9 go in 3 chunks or more
        case("syn_fd1_chunks", "synth16x8", 1, env=dict(ILQG_WORK_GB="0.00001")),
        case("syn_fd1_staged", "synth16x8", 1, staged=True),
        case("syn_fd0", "synth16x8", 0),
        case("synp_fd1", "synth16p", 1),
        case("synp_fd1_quad_stored", "synth16p", 1, env=dict(ILQG_QUAD_STORED="1")),
        case("syn10hx_fd1", "synth10hx", 1),
        case("car_wave", "carparking", 0, "wave"),
        case("syn_fd1_elem", "synth16x8", 1, "elem"),
        case("syn_fd1_lean", "synth16x8", 1, "lean"),
        case("syn_fd1_exp_deriv_parts", "synth16x8", 1, "exp", env=dict(ILQG_DERIV_PARTS="1")),
    ])


def big_case(cus):
    """a batch that fits the work buffer and fills the chip twice goes in two pieces (row mapping); ~160 MB of records"""
    return case("syn_fd0_two_pieces_rule", "synth16x8", 0, B=16 * cus + 9, n_hor=4, env=dict(ILQG_NO_QUAD="1"))


def inputs(pkg, c):
    """(params, opts, x0, u0, table) of a case"""
    B, n = c["B"], c["n_hor"]
    table = None
    if c["problem"] == "carparking":
        x0, u0 = pkg.synth.car_batch(B, n)
        params, opts = pkg.ilqg.CAR_PARAMS, {}
        if c["table"]:
            table = dict(cf=np.array(params["cf"]) * (1.0 + 0.01 * np.arange(B))[:, None])
    elif c["problem"] == "almix":
        params = dict(h=[0.1], cu=[0.05, 0.02], cx=[0.3, 0.05, 0.02], cf=[4.0, 1.0, 2.0], lim=[-1.1, 1.1], tgt=[2.0, 1.55, 0.45],
                      vref=0.8 + 0.4 * np.sin(np.arange(n + 1) * 0.2))
        opts = dict(w_pen_init_l=2.0, w_pen_init_f=2.0, w_pen_fact2=2.0, w_pen_max_l=200.0, w_pen_max_f=200.0)
        rng = np.random.default_rng(3)
        x0, u0 = np.array([0.0, 0.2, -0.3]) + 0.2 * rng.standard_normal((B, 3)), 0.1 * rng.standard_normal((B, n, 2))
    elif c["problem"] == "synth10hx":
        params, opts = SYN10_PARAMS, {}
        x0, u0 = syn10_inputs(B, n)
    else:
        params, opts = (SYNP_PARAMS_TIGHT if c["problem"] == "synth16p" else SYN_PARAMS_TIGHT), {}
        x0, u0 = syn_inputs(B, n)
    return params, dict(opts, max_iter=4, **c["opts"]), x0, u0, table


def run(pkg, c):
    """(arrays, launch counts) of a case; the caller has set the case's environment and unset the rest of ENV"""
    params, opts, x0, u0, table = inputs(pkg, c)
    s = pkg.ilqg.BatchSolver(c["problem"], c["fd"], batch=c["B"], n_hor=c["n_hor"], params=params, opts=opts, strict=c["build"], groups=c["groups"])
    try:
        if table:
            s.set_params_batch(table)
        s.timing(True)
        s.init(x0, u0)
        if c["staged"]:
            s.calc_derivs()
            s.back_pass()
            s.back_pass(single_sweep=True)
            s.back_pass(fused=True)
            s.line_search()
            s.update()
        else:
            s.iterate(2)
        out = dict(x=s.x(), u=s.u())
        out["l"], out["L"] = s.gains()
        for a in ARRAYS:
            out[a] = s.scalar(a)
        for a in INTS:
            out[a] = s.ints(a)
        counts = {k: n for k, (n, _) in s.kernel_times().items() if n}
    finally:
        s.close()
    return out, counts
