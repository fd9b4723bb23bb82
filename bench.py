#!/usr/bin/env python3
"""Benchmark: batched iLQG iterations/s on CarParking (n=4, m=2, N=500), 65 536
trajectories per GPU, fp64 (BASELINE.json metric).

    python bench.py --gpus 1 --steps 20 --warmup 2
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 \
        --master-port P bench.py --gpus N --steps K --warmup W

A "step" is one lock-step iLQG iteration of the whole batch: calc_derivs of the
nominal trajectories, back_pass (with its lambda retries), line_search over all 8
step sizes, accept/reject bookkeeping — for every trajectory.  The timed window
is the FIRST K iterations after the initial roll-out (no CarParking trajectory
converges before iteration 50, so all trajectories are active throughout).
Warm-up iterations run on the same inputs and the solver is then re-initialised
(untimed), so the timed work is always iterations 1..K.

One process per GPU; trajectories are independent, so ranks share nothing but a
single RCCL gather of the per-trajectory costs at the end of the timed window
(weak scaling: 65 536 trajectories per GPU).  PyTorch is used only for process
rendezvous, the RCCL collective and device synchronisation.

A plain run does what its headline needs: it sets up, warms up, times the K steps, writes --dump-outputs, and reports
what the timed window's own HIP events give.  Whatever takes runs of its own — the live PMC traffic, the CPU baseline,
the other configurations, the kernels alone, the full solves — is measured only with --full (a few minutes).

Prints ONE compact JSON line (rank 0; < 6 KB, nothing else reaches stdout) and writes the full report to
bench_detail.json beside this file (and to gpurun_out/ where that exists):
  value / ms_per_step   the timed window (three groups of trajectories on three streams)
  roofline              the dominant kernel's launches IN the timed window (HIP events on the solver's streams): SURVEY
                        8(d)'s algorithmic bytes of the stages it replaces / its average duration against 8 TB/s, the PMC
                        traffic per launch (the committed profiles/traffic.json; with --full collected in this run by
                        two short rocprofv3 child runs), its real HBM utilisation, the limiter and the issue counters of
                        the committed SQ passes
  iteration_roofline    the whole iteration against the HBM roofline with SURVEY 8(d)'s algorithmic bytes
  --full                adds, each reduced in the line and whole in bench_detail.json:
    cpu_baseline        the CPU checker (the reference's own sources when oracle/_ref was shipped) on a bounded
                        sample of the same workload on the host's cores
    config5, config5_stored, config2, dropin_b1
                        the other BASELINE configs, each measured in a fresh child process (`--object NAME`), reduced
                        to value / ms_per_step / fractions
    full_solve, roofline.alone, unfused_kernels
                        full solves to convergence, the dominant kernel alone and the unfused kernel pair
  --dump-outputs DIR    writes what the timed window computed (rank 0's shard) to DIR/*.npy: cost, lambda, status,
                        iterations of every trajectory, x / u of a fixed seeded sample of them (64 MB at most)
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

HBM_PEAK_GBS = 8000.0     # MI355X_MICROARCH.md: 8.0 TB/s spec (6.29 TB/s measured copy ceiling)
FP64_PEAK_TFLOPS = 78.6   # fp64 vector peak (spec; half the guide's FP32 vector 157.3 TF); v_fma_f64 measured at
                          # one per 2.6 ns and SIMD under load = 50 TFLOP/s (profiles/r2_ubench_dpp_row_fma.txt)


def tri(n):
    return n * (n + 1) // 2


def algorithmic_bytes(nx, nu, full):
    """per time step and trajectory, SURVEY.md §8(d) (doubles x 8 B)"""
    sxx, suu, nxu = tri(nx), tri(nu), nx * nu
    rec = nx + sxx + nu + suu + nxu + nx * nx + nxu + 2 * nu + (nx * (sxx + suu + nxu) if full else 0)
    b = {
        "k_derivs": (nx + nu + rec) * 8,
        "k_backward": (rec + nu + nu + nxu) * 8,
        "k_rollout[search]": (nx + 2 * nu + nxu) * 8,   # read once, shared by all step sizes
        "k_rollout[winner]": (nx + nu) * 8,             # the winner only is stored
    }
    b["iteration"] = sum(b.values())
    return b


def backpass_flops(n, m, full):
    """floating-point operations of ONE time step of the reference's back_pass (back_pass.c:80-251, matMult.c:3-72),
    a multiply-add counted as 2; the box QP with one factorisation (boxQP.c:75-232) and all inputs free."""
    sxx, suu, nm = tri(n), tri(m), n * m
    f = 2 * nm + 2 * n * n                                   # Qu, Qx (addMulVec)
    f += 2 * n * n * m + 2 * n * nm                          # Qxu (addMul2Tri: Vxx fu, then fx' that)
    f += 2 * n * n * m + 2 * n * m + (4 * n + 1) * (suu - m)  # Quu (addSquareTri)
    f += 2 * n * n * n + 2 * n * n + (4 * n + 1) * (sxx - n)  # Qxx (addSquareTri)
    if full:
        f += 2 * n * (sxx + suu + nm) + (sxx + suu + nm)     # sum_i Vx[i] * (fxx, fuu, fxu)_i
    f += 3 * (2 * m * m + 2 * m) + m ** 3 // 3 + 2 * m ** 3 + 4 * m * m  # box QP: values, gradient, factor, inverse, step
    f += 2 * m * m * n                                       # gains
    f += 2 * m + 2 * m * m + 3 * m                           # dV
    f += 2 * m * m + 2 * nm + 2 * nm + 2 * nm                # Vx
    f += 2 * m * m * n + 2 * m * n + (4 * m + 1) * (sxx - n) + 3 * n * n * m  # Vxx
    return f


def cpu_baseline(batch_per_gpu, iters, problem, fd, params, n_hor, make_inputs, budget_s=6.0, max_per_core=None):
    """CPU checker on a bounded sample of the same workload, one pthread per host core, each solving
    its share of the sample exactly as independent runs of the reference would (oracle/driver.c,
    drv_solve_many).  Returns the JSON object for `cpu_baseline`."""
    from oracle.harness import Driver, lib_path
    ref = lib_path("ref", problem, fd)
    kind = "reference" if os.path.exists(ref) else "port"
    path = ref if kind == "reference" else lib_path("oracle", problem, fd)
    cores = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1)
    d = Driver(path, n_hor, params, dict(max_iter=iters))
    # calibrate single-core speed on a few trajectories, then size the sample to the time budget
    ncal = 8 if problem == "carparking" else 1
    x0, u0 = make_inputs(ncal, n_hor)
    t0 = time.perf_counter()
    d.solve_many(x0, u0, 1)
    per_traj = max((time.perf_counter() - t0) / ncal, 1e-5)
    # threads on a loaded many-core host run ~2-3x slower than the single calibration thread: the budget is
    # sized for ~10-20 s of wall time
    sample = int(max(cores, min(32768, budget_s / per_traj * cores)))
    if max_per_core:  # large problems: the threads share the memory bandwidth and run far slower than the calibration
        sample = min(sample, max_per_core * cores)
    x0, u0 = make_inputs(sample, n_hor)
    t0 = time.perf_counter()
    cost, its, rc = d.solve_many(x0, u0, cores)
    dt = time.perf_counter() - t0
    d.close()
    traj_iters_per_s = float(its.sum()) / dt
    return {
        "value": traj_iters_per_s / batch_per_gpu,  # batched iterations/s of a whole-batch equivalent
        "unit": "iterations/s (%d-trajectory batch equivalent)" % batch_per_gpu,
        "cores": cores,
        "kind": kind,
        "single_core_ms_per_trajectory_iteration": 1e3 * per_traj / iters,
        "sample": "%d trajectories x %d iterations (same generator, trajectories 0..%d) in %.1f s on %d threads; "
                  "%.0f trajectory-iterations/s" % (sample, iters, sample - 1, dt, cores, traj_iters_per_s),
    }


def stamped(name):
    """a committed profile (profiles/<name>) if it was collected on the current kernel sources, else (None, why):
    ddp-generator_amd/evidence.py"""
    import __graft_entry__ as g
    ev = g.load_package().evidence
    return ev.load_stamped(os.path.join(ROOT, "profiles", name))


def issue_object(kernel, name="issue.json"):
    """roofline.issue: what actually bounds the sweep kernels — vector instructions per step and how much of a wavefront's
    time goes into issuing them (committed SQ counter passes, tools/round_profile.sh)"""
    j, why = stamped(name)
    if j is None:
        return {"valu_insts_per_step": None, "active_valu_frac": None, "source": None, "stale": why}
    k = j.get(kernel)
    if not k:  # (a kernel template that has gained a parameter: "k_backward_quad<true>" also means "k_backward_quad<true, true>")
        alt = [n for n in j if isinstance(j[n], dict) and n.startswith(kernel[:-1] + ",")]
        if len(alt) == 1:
            kernel, k = alt[0], j[alt[0]]
    if not k:
        return {"valu_insts_per_step": None, "active_valu_frac": None, "source": "profiles/" + name, "stale": "no entry for " + kernel}
    if "valu_insts_per_trajectory_step" not in k and k.get("persistent"):
        # a persistent kernel's wavefronts walk many trajectories and sweeps: instructions / (wavefronts x n_hor) means
        # nothing; only the profile build's count of the steps walked (--wave-steps) makes a per-step figure
        return {"kernel": kernel, "valu_insts_per_step": None, "active_valu_frac": k["active_valu_frac"], "wait_any_frac": k.get("wait_any_frac"),
                "source": "profiles/" + name, "stale": "no step count of the persistent kernel in this file (tools/round_profile.sh, --wave-steps)"}
    per_step = k.get("valu_insts_per_trajectory_step", k.get("valu_insts_per_wave_and_step"))
    return {"kernel": kernel, "valu_insts_per_step": per_step, "active_valu_frac": k["active_valu_frac"],
            "per": ("step of a trajectory: wavefront instructions over the steps the wavefronts walked (%.0f per wavefront step, counted "
                    "by the profile build of the same sources) / %d trajectories per wavefront" % (k["valu_insts_per_wavefront_step"], k["trajectories_per_wavefront"]))
                   if "valu_insts_per_trajectory_step" in k else "step of a wavefront",
            "wait_any_frac": k.get("wait_any_frac"), "valu_insts_total": k.get("valu_insts_total"),
            "source": "profiles/%s (rocprofv3 --pmc SQ_INSTS_VALU / SQ_WAVES / %d steps; SQ_ACTIVE_INST_VALU / SQ_WAVE_CYCLES; sources %s; "
                      "not collected in this run)" % (name, j.get("_steps", 0), j.get("_source_sha"))}


def live_traffic(workload_args, labels=True, timeout=240):
    """HBM bytes per launch of the benchmark's kernels, collected NOW: two rocprofv3 --pmc passes (FETCH_SIZE, WRITE_SIZE — separate
    passes, the guide's gfx950 corrections: FETCH_SIZE x 2, both KiB) of a short run of this script in child processes, summarised by
    tools/pmc_summary.py's rule.  Returns ({label: bytes per launch}, detail) or (None, why)."""
    import shutil
    import subprocess
    import tempfile
    if not shutil.which("rocprofv3"):
        return None, "rocprofv3 not on PATH"
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import pmc_summary
    out = tempfile.mkdtemp(prefix="ilqg_traffic_", dir="/tmp")
    try:
        dirs = []
        for c in ("FETCH_SIZE", "WRITE_SIZE"):
            d = os.path.join(out, c)
            cmd = ["rocprofv3", "--pmc", c, "--kernel-trace", "--output-format", "csv", "-d", d, "--", sys.executable, os.path.abspath(__file__),
                   "--steps", "3", "--warmup", "0", "--no-cpu-baseline", "--no-unfused", "--no-live-traffic"] + workload_args
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=timeout, cwd="/tmp", env=dict(os.environ, TMPDIR="/tmp"))
            if r.returncode != 0:
                return None, "rocprofv3 --pmc %s failed: %s" % (c, (r.stderr or r.stdout)[-300:])
            dirs.append(d)
        tj = os.path.join(out, "traffic.json")
        argv = sys.argv
        try:
            sys.argv = ["pmc_summary.py", "--traffic-json", tj] + dirs
            import io, contextlib
            with contextlib.redirect_stdout(io.StringIO()):
                pmc_summary.main()
        finally:
            sys.argv = argv
        j = json.load(open(tj))
        return j, ("collected in this run: rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE (separate passes) of `bench.py --steps 3 --warmup 0 "
                   "--no-unfused` in child processes; FETCH_SIZE x2 + WRITE_SIZE, KiB -> bytes, mean per launch")
    except Exception as e:  # the line must not depend on the profiler
        return None, "%s: %s" % (type(e).__name__, e)
    finally:
        shutil.rmtree(out, ignore_errors=True)


def with_split(opts, args):
    """the solver options of a run: the library's line-search split unless --ls-split asks for another"""
    if args.ls_split is not None:
        opts["ls_split"] = args.ls_split
    return opts


def kernel_alone(ilqg, problem, fd, B, n_hor, params, x0, u0, local, iters, **opts):
    """{kernel: (launches, total ms)} of `iters` iterations run as ONE group of trajectories: every launch covers the
    whole batch and nothing else is on the GPU while it is timed"""
    s = ilqg.BatchSolver(problem, fd, batch=B, n_hor=n_hor, device=local, params=params,
                         opts=dict(max_iter=iters + 1, **opts), groups=1)
    s.init(x0, u0)
    s.timing(True)
    s.iterate(iters)
    s.sync()
    t = s.kernel_times()
    s.close()
    return t


CONFIG5_VARIANTS = {
    # problem library, committed PMC passes, issue figures, kernels, mapping
    "factored": ("synth16x8", "traffic_config5.json", ("k_backward_quad<true>", "issue_config5.json"),
                 "k_derivs_wave + k_backward_quad + roll-outs",
                 "quad mapping: 16 lanes per trajectory in the backward step, four trajectories per wavefront, "
                 "each 16-lane row a worker that takes trajectories from a queue (k_backward_quad); records carry "
                 "the first-order derivatives and the 32 products the tensors are multiples of (factored tensor "
                 "tables of the generated file), written as whole cache lines from LDS (k_derivs_wave), the "
                 "backward step multiplies the tensors out"),
    # the same problem emitted WITHOUT any additive hint or table (tools/gen_problem.py --plain): what a
    # Maxima / gentran-written pair looks like to the kernels — every tensor entry stored in the record and read back
    "stored": ("synth16x8_plain", "traffic_config5_stored.json", ("k_backward_wave<false>", "issue_config5_stored.json"),
               "k_derivs_wave<false> + k_backward_wave<false> + roll-outs",
               "row mapping: one wavefront per trajectory in the backward step (k_backward_wave), records are the "
               "reference's trajEl_t with the tensors fxx / fuu / fxu stored by the generated bp_derivsL (47.9 KB per "
               "step) and contracted from HBM (back_pass.c:95-131): the path of a generated pair without hints"),
    # the n = 16 problem with pairwise state products in the nonlinearity (problems/defs/synth16p.py): the generator's
    # hints are there (roll-outs in parts) but the tensors do not factor — stored tensors again
    "pair": ("synth16p", "traffic_config5_pair.json", ("k_backward_wave<false>", "issue_config5_pair.json"),
             "k_derivs_wave<false> + k_backward_wave<false> + roll-outs in parts",
             "row mapping, stored tensors (the second derivatives of f_i are not multiples of one product: no tables)"),
}


def config5(ilqg, synth, local, K=3, W=1, with_cpu=True, variant="factored"):
    """BASELINE config 5: synthetic n=16, m=8, N=1000, FULL_DDP=1, 16 384 trajectories (wave mapping: 16 lanes per trajectory).
    variant "stored": the hint-free pair of the same problem (stored tensors)"""
    B, N, nx, nu = 16384, 1000, 16, 8
    problem, traffic_file, (issue_kernel, issue_file), kernels_label, mapping = CONFIG5_VARIANTS[variant]
    alg = algorithmic_bytes(nx, nu, 1)
    x0, u0 = synth.synth16_batch(B, N)
    params = dict(synth.SYNTH16_PARAMS, e=[0.3]) if variant == "pair" else synth.SYNTH16_PARAMS
    s = ilqg.BatchSolver(problem, 1, batch=B, n_hor=N, device=local, params=params,
                         opts=dict(max_iter=K + W + 1))
    s.init(x0, u0)
    if W > 0:
        s.iterate(W)
        s.sync()
        s.init(x0, u0)
    s.timing(True)
    s.sync()
    t0 = time.perf_counter()
    s.iterate(K)
    s.sync()
    dt = time.perf_counter() - t0
    times = s.kernel_times()
    busy = s.kernel_busy()
    sweeps = float(s.ints("bp_calls").mean())
    active = s.active()
    cost = float(s.scalar("cost").mean())
    s.close()
    it_s = K / dt
    iter_bytes = alg["iteration"] * N * B
    flops = backpass_flops(nx, nu, 1) * N * B  # one sweep per iteration; lambda retries repeat (parts of) it
    # what an iteration really moves: PMC passes of `bench.py --workload synth` (tools/round_profile.sh), committed
    traffic, traffic_detail = None, None
    tj, why = stamped(traffic_file)
    if tj is None:
        traffic_detail = {"stale": why}
    else:
        traffic = tj["iteration"]["hbm_bytes"]
        traffic_detail = {"source": "profiles/%s (rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE passes of "
                                    "`bench.py --workload synth`, FETCH_SIZE x2 + WRITE_SIZE, every kernel of an iteration; sources "
                                    "%s; not collected in this run)" % (traffic_file, tj.get("_source_sha")),
                          "hbm_GBs": traffic * it_s / 1e9, "hbm_frac_of_peak": traffic * it_s / 1e9 / HBM_PEAK_GBS,
                          "per_kernel": {k: {"hbm_bytes_per_iteration": v["hbm_bytes_per_launch"] * v["launches_per_iteration"]}
                                         for k, v in tj.items() if k not in ("iteration", "_source_sha")}}
    out = {
        "metric": "iLQG iterations/sec, batch 16384 synthetic problem (n=16,m=8,N=1000, FULL_DDP=1)",
        "value": it_s, "unit": "iterations/s", "steps": K, "warmup": W, "ms_per_step": 1e3 * dt / K, "dtype": "f64",
        "config": {"workload": "Synth16x8 batch=16384, 8-alpha line search, FULL_DDP=1, first %d iterations after the "
                               "initial roll-out" % K,
                   "problem_library": problem, "mapping": mapping,
                   "backward_sweeps_per_trajectory_in_last_iteration": sweeps},
        # frac / achieved: what the iteration REALLY moves (PMC bytes of the committed passes x iterations/s) against the
        # peak — a utilisation.  The contract's algorithmic figure (SURVEY 8(d)'s bytes with every tensor materialised) is
        # an HBM-EQUIVALENT and sits beside it under its own name: the factored path never moves those bytes, so it may
        # pass 1.
        "roofline": {"bound": "hbm", "kernel": "iteration (%s)" % kernels_label,
                     "achieved": (traffic * it_s / 1e9) if traffic else None, "peak": HBM_PEAK_GBS, "unit": "GB/s",
                     "frac": (traffic * it_s / 1e9 / HBM_PEAK_GBS) if traffic else None,
                     "frac_kind": "HBM utilisation: PMC bytes per iteration (`traffic`) x iterations/s / peak" if traffic else
                                  "null: no PMC traffic collected on these sources (traffic_detail.stale); see hbm_equivalent_frac",
                     "traffic": traffic, "traffic_detail": traffic_detail,
                     "hbm_equivalent_GBs": iter_bytes * it_s / 1e9, "hbm_equivalent_frac": iter_bytes * it_s / 1e9 / HBM_PEAK_GBS,
                     "algorithmic_bytes_per_iteration": iter_bytes,
                     "note": "hbm_equivalent_*: SURVEY 8(d)'s 91 200 algorithmic bytes per step and trajectory with the "
                             "tensors materialised (1.49 TB per iteration, ceiling 5.4 it/s) x iterations/s — the contract's "
                             "recipe; with factored tensors the path moves ~7 KB per step instead of 44 KB, so the equivalent "
                             "is not a utilisation.  Kernel launches of consecutive chunks overlap on two streams, so no "
                             "per-launch figure is given.",
                     "backward_fp64": {"algorithmic_TFLOPs": flops * it_s / 1e12, "peak": FP64_PEAK_TFLOPS,
                                       "frac": flops * it_s / 1e12 / FP64_PEAK_TFLOPS,
                                       "note": "reference back_pass arithmetic, one sweep per iteration, over the WHOLE "
                                               "iteration time"}},
        # wall clock each kernel occupied per iteration: the union of its launch intervals (the two pieces of the batch run
        # on two streams and take turns on the chip; the plain sum of their event spans counts the waiting twice)
        "kernels_busy_ms_per_iteration": {k: v / K for k, v in busy.items()},
        "kernels_ms_per_iteration_sum_of_spans": {k: v[1] / K for k, v in times.items() if v[0]},
        "trajectories_still_active": int(active), "cost_mean_after_window": cost,
    }
    out["roofline"]["issue"] = issue_object(issue_kernel, issue_file)
    if with_cpu:
        out["cpu_baseline"] = cpu_baseline(B, K, "synth16x8", 1, synth.SYNTH16_PARAMS, N, synth.synth16_batch, budget_s=4.0,
                                           max_per_core=2)
    return out


def config2(ilqg, synth, local, K=20, W=2):
    """BASELINE config 2: CarParking, 4 096 randomised starts, fp64, one GPU — in the lane mapping (the product's choice
    for n <= 8) and in the one-wavefront-per-trajectory build BASELINE.json words it for"""
    B, N = 4096, 500
    x0, u0 = synth.car_batch(B, N)
    out = {"metric": "iLQG iterations/sec, batch 4096 CarParking (n=4,m=2,N=500)", "unit": "iterations/s", "steps": K, "warmup": W,
           "config": {"workload": "CarParking batch=4096 randomised x0, 8-alpha line search, FULL_DDP=0, first %d iterations after "
                                  "the initial roll-out" % K}}
    for label, variant in (("lane_mapping", False), ("wave_mapping", "wave")):
        s = ilqg.BatchSolver("carparking", 0, batch=B, n_hor=N, device=local, params=ilqg.CAR_PARAMS, opts=dict(max_iter=K + W + 1),
                             strict=variant)
        s.init(x0, u0)
        if W > 0:
            s.iterate(W)
            s.sync()
            s.init(x0, u0)
        s.sync()
        t0 = time.perf_counter()
        s.iterate(K)
        s.sync()
        dt = time.perf_counter() - t0
        out[label] = {"value": K / dt, "ms_per_step": 1e3 * dt / K, "stream_groups": s.groups(),
                      "cost_mean_after_window": float(s.scalar("cost").mean()), "trajectories_still_active": int(s.active())}
        s.close()
    out["note"] = ("4 096 trajectories are 64 wavefronts in the lane mapping (a 16th of the chip's SIMDs, each a chain of 500 "
                   "dependent steps: the time is that of ONE wavefront's chain) and 4 096 wavefronts in the wave mapping")
    return out


def dropin_b1(ilqg, synth, iters=20):
    """BASELINE config 1 through the drop-in iLQG(): one CarParking trajectory, the reference's demo start"""
    x0, u0 = synth.car_single()
    ilqg.solve_single(x0, u0, ilqg.CAR_PARAMS, dict(max_iter=2))  # first call: context, buffers
    r = ilqg.solve_single(x0, u0, ilqg.CAR_PARAMS, dict(max_iter=iters))
    n = max(1, r["iterations"])
    return {"ms_per_iteration": 1e3 * r["seconds"] / n, "iterations": r["iterations"], "cost": r["cost"],
            "note": "ilqg_solve_single (the MEX entry's call sequence): outer loop and calc_derivs on the host, back_pass() "
                    "and line_search() on the GPU with a batch of one; a 500-step sweep is a chain of dependent steps, "
                    "so one trajectory cannot use the GPU — compare cpu_baseline.single_core_ms_per_trajectory_iteration"}


def solve_once(ilqg, synth, local, B, n_hor, max_iter, compact):
    """one full solve of B CarParking starts in THIS process (see full_solve): seconds, trace, per-start results"""
    x0, u0 = synth.car_batch(B, n_hor)
    s = ilqg.BatchSolver("carparking", 0, batch=B, n_hor=n_hor, device=local, params=ilqg.CAR_PARAMS, opts=dict(max_iter=max_iter, compact=compact))
    s.init(x0, u0)
    s.sync()
    t0 = time.perf_counter()
    s.solve()
    s.sync()
    dt = time.perf_counter() - t0
    it, act, slots, ncomp = s.solve_trace()
    status, iters, cost = s.ints("status"), s.ints("iterations"), s.scalar("cost")
    s.close()
    import hashlib
    digest = hashlib.sha256(status.tobytes() + iters.tobytes() + cost.tobytes()).hexdigest()[:16]
    steps = np.diff(np.concatenate([[0], it]))              # iterations each poll covered
    before = np.concatenate([[B], act[:-1]])                  # live when those iterations started
    q = np.percentile(iters, [5, 25, 50, 75, 95])
    names = {1: "gradient test", 2: "cost test", 3: "max_iter", 4: "lambda > lambdaMax (backward pass)", 5: "lambda > lambdaMax (rejected step)",
             6: "NaN/Inf in derivatives", 7: "initial roll-out failed", 0: "still active"}
    return {"seconds": dt, "value": B / dt, "iterations_run": int(it[-1]), "compactions": ncomp,
            "slot_iterations": int((slots * steps).sum()), "live_lane_iterations_upper_bound": int((before * steps).sum()),
            "lane_occupancy": float((before * steps).sum() / max(1, (slots * steps).sum())),
            "occupancy_over_time": [{"iteration": int(a), "active": int(b), "slots": int(c)} for a, b, c in
                                    list(zip(it, act, slots))[::max(1, len(it) // 16)]],
            "results_digest": digest,
            "iterations_per_start": {"min": int(iters.min()), "p5": q[0], "p25": q[1], "median": q[2], "p75": q[3], "p95": q[4],
                                     "max": int(iters.max()), "mean": float(iters.mean())},
            "exits": {names.get(int(k), str(k)): int(v) for k, v in zip(*np.unique(status, return_counts=True))},
            "cost_mean": float(cost.mean())}


def solve_stream_once(ilqg, synth, local, B, n_hor, max_iter, total):
    """`total` CarParking starts streamed through B resident slots (ilqg_batch_solve_stream) in THIS process: the starts
    come from host memory (x0, u0 of every refill cross PCIe inside the timed region), cost / exit / iterations go back"""
    x0, u0 = synth.car_batch(total, n_hor)
    s = ilqg.BatchSolver("carparking", 0, batch=B, n_hor=n_hor, device=local, params=ilqg.CAR_PARAMS, opts=dict(max_iter=max_iter))
    s.sync()
    t0 = time.perf_counter()
    r = s.solve_stream(x0, u0)
    s.sync()
    dt = time.perf_counter() - t0
    it, act, slots, refills = s.solve_trace()
    s.close()
    import hashlib
    digest_first_batch = hashlib.sha256(r["status"][:B].tobytes() + r["iterations"][:B].tobytes() + r["cost"][:B].tobytes()).hexdigest()[:16]
    steps = np.diff(np.concatenate([[0], it]))
    return {"seconds": dt, "value": total / dt, "starts": total, "resident_slots": B, "iterations_run": int(it[-1]), "refills": refills,
            "lane_occupancy": float((act[1:] * steps[1:]).sum() / max(1, (slots[1:] * steps[1:]).sum())) if len(it) > 1 else None,
            "results_digest_of_the_first_%d_starts" % B: digest_first_batch,
            "iterations_mean": float(r["iterations"].mean()), "cost_mean": float(r["cost"].mean()),
            "inputs": "host memory: x0 / u0 of every refill cross PCIe inside the timed region (%.2f GB in all)" % (u0.nbytes / 1e9)}


def full_solve(local, B=65536, n_hor=500, max_iter=500, compact=2048):
    """The reference's product — a solve to convergence (iLQG.c:224-379) — for a batch of CarParking starts: solves/s with
    and without retiring finished trajectories (option "compact": the live trajectories are gathered into smaller contexts,
    ilqg_host.c ilqg_batch_solve), the iterations the starts need, and how many of the lanes the iterations ran over were
    live.  The same starts, the same results bit for bit (digest of cost / status / iterations).  Each solve runs in a
    process of its own: a context that shares the process with another one — or follows one that was released — has been
    measured up to 50 % slower per iteration (the streams of all contexts share the process's four hardware queues)."""
    import subprocess
    out = {"metric": "iLQG solves/sec, %d CarParking starts (n=4,m=2,N=%d), max_iter %d" % (B, n_hor, max_iter), "unit": "solves/s",
           "config": {"workload": "CarParking batch=%d randomised x0 (the benchmark's generator), u0 = 0.1 N(0,1), solved to the reference's "
                                  "exit tests (iLQG.c:297-303, :331, :365-378), max_iter %d (testCar.m:19 has 200), default options" % (B, max_iter),
                      "compact_min_trajectories": compact}}
    for label, cmin in (("plain", 0), ("compacted", compact)):
        cmd = [sys.executable, os.path.abspath(__file__), "--solve-one", str(cmin), "--batch", str(B), "--n-hor", str(n_hor), "--max-iter", str(max_iter)]
        env = dict(os.environ, ILQG_DEVICE_ORDINAL=str(local))
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, env=env)
        lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
        if r.returncode != 0 or not lines:
            raise RuntimeError("%s solve failed: %s" % (label, r.stderr[-500:]))
        out[label] = json.loads(lines[-1])
    # a stream of 3 x B starts through the B slots (ilqg_batch_solve_stream): finished slots are refilled
    cmd = [sys.executable, os.path.abspath(__file__), "--solve-stream", str(3 * B), "--batch", str(B), "--n-hor", str(n_hor), "--max-iter", str(max_iter)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=900, env=dict(os.environ, ILQG_DEVICE_ORDINAL=str(local)))
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    out["streamed"] = json.loads(lines[-1]) if r.returncode == 0 and lines else {"error": r.stderr[-500:]}
    if "value" in out["streamed"]:
        out["streamed"]["first_batch_identical_to_plain"] = out["streamed"]["results_digest_of_the_first_%d_starts" % B] == out["plain"]["results_digest"]
    for k in ("iterations_per_start", "exits", "cost_mean"):
        out[k] = out["plain"].pop(k)
        out["compacted"].pop(k)
    out["compacted"]["identical_to_plain"] = out["compacted"]["results_digest"] == out["plain"]["results_digest"]
    out["value"] = max(out["compacted"]["value"], out["streamed"].get("value", 0.0))
    out["speedup_from_compaction"] = out["compacted"]["value"] / out["plain"]["value"]
    if "value" in out["streamed"]:
        out["speedup_from_streaming"] = out["streamed"]["value"] / out["plain"]["value"]
    out["note"] = ("retiring finished trajectories raises the share of live lanes among the lanes iterated (lane_occupancy) but hardly the "
                   "rate: an iteration of a few thousand CarParking trajectories takes what an iteration of 65 536 takes — the chains of "
                   "n_hor dependent steps of its backward sweep and two search stages, one wavefront per SIMD either way")
    return out


class ProtocolShard:
    """--rehearse-protocol: stands where the solver of a rank stands and does NO numerics — its "costs" are the global
    indices of the shard's trajectories.  What runs for real is everything around the solver in main(): the shard
    offsets, the barriers on both sides of the timed region, the single gather of the per-trajectory costs, the maximum
    over the ranks, the assembly of the JSON line on rank 0.  For boxes without a GPU (the line says `rehearsal`; its
    `value` is not a measurement)."""

    class _Problem:
        wave_mapping = False

    problem = _Problem()

    def __init__(self, B, first):
        self.B, self.first, self.iters = B, first, 0

    def init(self, x0, u0):
        assert len(x0) == self.B and len(u0) == self.B
        self.iters = 0

    def iterate(self, n):
        self.iters += n

    def sync(self):
        pass

    def timing(self, enable=True):
        pass

    def set_option(self, name, value):
        pass

    def scalar(self, name):
        return np.arange(self.first, self.first + self.B, dtype=np.float64) + 0.001 * self.iters

    def kernel_times(self):
        return {}

    def active(self):
        return self.B

    def groups(self):
        return 1

    def close(self):
        pass


def single_process(args, ilqg, synth, guard):
    """N GPUs of the node driven by ONE process through ilqg_multi_* (the C counterpart of the torchrun path);
    --devices 0,0,...: the shards on the listed devices (equal ids: loop-back rehearsal on one GPU)"""
    G, K, W = args.gpus, args.steps, args.warmup
    per, n_hor = (args.batch or 65536), (args.n_hor or 500)
    B = per * G
    devices = [int(v) for v in args.devices.split(",")] if args.devices else list(range(G))
    assert len(devices) == G, "--devices needs one id per shard (--gpus %d)" % G
    x0, u0 = synth.car_batch(B, n_hor)
    m = ilqg.MultiSolver("carparking", 0, batch=B, n_hor=n_hor, devices=devices, params=ilqg.CAR_PARAMS,
                         opts=with_split(dict(max_iter=max(K, W) + 1), args))
    m.init(x0, u0)
    if W > 0:
        m.iterate(W)
        m.sync()
        m.init(x0, u0)
    m.sync()
    t0 = time.perf_counter()
    m.iterate(K)
    cost = m.costs()  # the single collective (ncclGather), synchronises
    m.sync()
    dt = time.perf_counter() - t0
    active = m.active()
    if args.dump_outputs:
        dump_outputs(args.dump_outputs, {"cost": cost, **{k: m.ints(k) for k in ("status", "iterations")}}, m.x, m.u)
    m.close()
    iter_bytes = algorithmic_bytes(4, 2, 0)["iteration"] * n_hor * per
    out = {
        "metric": "iLQG iterations/sec, 65k-batch CarParking (n=4,m=2,N=500)", "value": G * K / dt,
        "unit": "iterations/s", "value_definition": "iterations of a %d-trajectory batch per second, all shards: %d x %d iterations / time" % (per, G, K),
        "per_gpu_iterations_per_s": K / dt,
        "n_gpus": G, "steps": K, "warmup": W, "ms_per_step": 1e3 * dt / K, "higher_is_better": True, "scaling": "weak",
        "vs_baseline": None, "dtype": "f64", "data": "synthetic",
        "config": {"workload": "CarParking batch=%d per GPU x %d GPU, 8-alpha line search, FULL_DDP=0, first %d iterations "
                               "after the initial roll-out" % (per, G, K),
                   "batch_per_gpu": per, "n_hor": n_hor,
                   "devices": devices,
                   "parallelism": "ONE process, ilqg_multi_*: contiguous shards, one ncclGather of the costs"
                                  + (" (all shards on one device: the gather is device-to-device copies)" if len(set(devices)) == 1 and G > 1 else "")},
        "roofline": {"bound": "hbm", "kernel": "iteration", "achieved": iter_bytes * (K / dt) / 1e9, "peak": HBM_PEAK_GBS,
                     "unit": "GB/s", "frac": iter_bytes * (K / dt) / 1e9 / HBM_PEAK_GBS, "traffic": None,
                     "note": "per GPU; algorithmic bytes of SURVEY 8(d)"},
        "trajectories_still_active": int(active), "cost_mean_after_window": float(cost.mean())}
    out["detail"] = write_detail(out)
    guard.emit(json.dumps(out))


# ---------------------------------------------------------------------------------------------------------------------
# Output: ONE compact JSON line on stdout (what the driver parses: < 6 KB, tests/test_multiproc.py asserts it), the full
# report in bench_detail.json beside this file (and under gpurun_out/ where that exists).  Everything else that would
# reach stdout — console lines of C libraries, of child processes — is kept off it: fd 1 points at bench_detail.log while
# the benchmark runs and is put back for the one line.

LINE_CAP = 6000


class StdoutGuard:
    """fd 1 -> a log file for the duration of the run (C printf of the checker libraries included); emit() writes the
    one line to the real stdout"""

    def __init__(self):
        sys.stdout.flush()
        self.real = os.dup(1)
        log = None
        for d in (ROOT, "/tmp"):
            try:
                log = os.open(os.path.join(d, "bench_detail.log"), os.O_WRONLY | os.O_CREAT | os.O_TRUNC, 0o644)
                break
            except OSError:
                continue
        if log is None:
            log = os.open(os.devnull, os.O_WRONLY)
        os.dup2(log, 1)
        os.close(log)

    def emit(self, line):
        sys.stdout.flush()
        os.dup2(self.real, 1)
        os.write(1, (line + "\n").encode())


def write_detail(out):
    """the full report: bench_detail.json beside bench.py, and in gpurun_out/ so that it comes back from a GPU box"""
    paths = [os.path.join(ROOT, "bench_detail.json")]
    if os.path.isdir(os.path.join(ROOT, "gpurun_out")):
        paths.append(os.path.join(ROOT, "gpurun_out", "bench_detail.json"))
    written = None
    for p in paths:
        try:
            with open(p, "w") as f:
                json.dump(out, f, indent=1)
            written = written or os.path.relpath(p, ROOT)
        except OSError:
            pass
    return written


DUMP_CAP = 64 * 10 ** 6  # bytes, all files of --dump-outputs together
DUMP_SEED = 5


def dump_outputs(directory, per_trajectory, get_x, get_u):
    """--dump-outputs DIR: what the timed window computed, as DIR/<name>.npy in float64, so that two builds can be compared
    output for output on the same inputs.  per_trajectory: {name: [B] array} of every trajectory (cost, lambda, status,
    iterations); get_x / get_u: the solver's state and control trajectories [B, N+1, n_x] / [B, N, n_u], of which a fixed,
    seeded sample of trajectories is written (x.npy, u.npy, their indices in sample.npy) so that the whole stays under
    DUMP_CAP bytes"""
    os.makedirs(directory, exist_ok=True)
    arrays = {k: np.asarray(v, dtype=np.float64) for k, v in per_trajectory.items()}
    x, u = get_x(), get_u()
    B = x.shape[0]
    row = (x[0].size + u[0].size + 1) * 8
    room = DUMP_CAP - sum(a.nbytes for a in arrays.values()) - 4096 * (len(arrays) + 3)  # (npy headers)
    n = max(0, min(B, room // row))
    sample = np.sort(np.random.default_rng(DUMP_SEED).choice(B, n, replace=False)) if n < B else np.arange(B)
    arrays.update(x=x[sample], u=u[sample], sample=sample.astype(np.float64))
    for k, v in arrays.items():
        np.save(os.path.join(directory, k + ".npy"), np.ascontiguousarray(v))
    assert sum(os.path.getsize(os.path.join(directory, k + ".npy")) for k in arrays) <= DUMP_CAP


def _pick(d, *keys):
    return {k: d[k] for k in keys if isinstance(d, dict) and k in d}


def compact_line(out, detail_path):
    """the line the driver parses, cut down from the full report `out` (the contract's keys, the dominant kernel's
    roofline, the CPU baseline, the other configs as value / ms_per_step / fractions); never longer than LINE_CAP"""
    c = out.get("config", {})
    line = _pick(out, "metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling",
                 "vs_baseline", "dtype", "data", "rehearsal", "gathered_costs_in_order", "per_gpu_iterations_per_s",
                 "trajectories_still_active", "cost_mean_after_window")
    line["config"] = _pick(c, "workload", "mapping", "batch_per_gpu", "n_hor", "full_ddp", "stream_groups", "parallelism", "device_ordinal_of_rank_0", "device_note")
    if out.get("collective"):
        line["collective"] = out["collective"]
    rf = out.get("roofline", {})
    r = _pick(rf, "bound", "kernel", "achieved", "peak", "unit", "frac", "traffic", "hbm_utilisation_frac", "limiter")
    dl = rf.get("dominant_launch") or {}
    r.update({k: dl[k] for k in ("avg_launch_ms", "launches", "trajectories_per_launch") if k in dl})
    if "hbm_equivalent" in dl:
        r["algorithmic_bytes_per_launch"] = dl["hbm_equivalent"]["algorithmic_bytes_per_launch"]
    if "valu_fp64" in dl:
        r["valu_fp64_frac"] = dl["valu_fp64"]["frac_of_peak"]
    if dl.get("pmc", {}).get("source"):
        r["traffic_source"] = "live" if dl["pmc"]["source"].startswith("collected in this run") else "profiles/traffic.json"
    iss = rf.get("issue") or {}
    r.update({k: iss[k] for k in ("valu_insts_per_step", "active_valu_frac") if iss.get(k) is not None})
    if rf.get("alone"):
        r["alone_avg_launch_ms"] = rf["alone"]["avg_launch_ms"]
    line["roofline"] = r
    ir = out.get("iteration_roofline")
    if ir:
        line["iteration_roofline"] = {"achieved": ir["achieved_GBs"], "frac": ir["frac_of_peak"], "unit": "GB/s",
                                      "algorithmic_bytes_per_iteration": ir["algorithmic_bytes_per_iteration"]}
    if out.get("cpu_baseline"):
        line["cpu_baseline"] = out["cpu_baseline"]
    for name in ("config5", "config5_stored"):
        o = out.get(name)
        if not o:
            continue
        if "error" in o:
            line[name] = {"error": str(o["error"])[:160]}
            continue
        orf = o.get("roofline", {})
        line[name] = {"value": o["value"], "ms_per_step": o["ms_per_step"], "steps": o["steps"], "frac": orf.get("frac"),
                      "hbm_equivalent_frac": orf.get("hbm_equivalent_frac"), "traffic": orf.get("traffic"),
                      "active_valu_frac": (orf.get("issue") or {}).get("active_valu_frac")}
        if o.get("cpu_baseline"):
            line[name]["cpu_baseline_value"] = o["cpu_baseline"]["value"]
    o = out.get("config2")
    if o:
        line["config2"] = {"error": str(o["error"])[:160]} if "error" in o else \
            {k: o[k]["value"] for k in ("lane_mapping", "wave_mapping") if k in o}
    o = out.get("dropin_b1")
    if o:
        line["dropin_b1"] = _pick(o, "ms_per_iteration", "iterations") if "error" not in o else {"error": str(o["error"])[:160]}
    o = out.get("full_solve")
    if o:
        line["full_solve"] = _pick(o, "value", "unit", "speedup_from_compaction", "speedup_from_streaming") if "error" not in o \
            else {"error": str(o["error"])[:160]}
    line["detail"] = detail_path
    # the cap holds whatever a run put into the report: optional objects go first, the contract's keys never
    for k in ("full_solve", "dropin_b1", "config2", "collective", "iteration_roofline", "config5_stored", "config5"):
        if len(json.dumps(line)) < LINE_CAP:
            break
        line.pop(k, None)
    s = json.dumps(line)
    assert len(s) < LINE_CAP, len(s)
    return s


def run_object(name, local, extra=(), timeout=900):
    """a secondary object of the report measured in a FRESH child process (`bench.py --object NAME`, started with
    subprocess — never an exec of this GPU-initialised process): its own HIP context and hardware queues, its buffers
    allocated into an empty device, so that its numbers do not depend on what ran before it in this process"""
    import subprocess
    cmd = [sys.executable, os.path.abspath(__file__), "--object", name] + [str(a) for a in extra]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=timeout, env=dict(os.environ, ILQG_DEVICE_ORDINAL=str(local)))
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    if r.returncode != 0 or not lines:
        return {"error": "child `--object %s` rc %d: %s" % (name, r.returncode, (r.stderr or r.stdout)[-300:])}
    return json.loads(lines[-1])


def child_object(args):
    """`--object NAME`: one secondary object in this (fresh) process, as one JSON line"""
    import __graft_entry__ as g
    g.load_package()
    from ddp_generator_amd import ilqg, synth
    local = int(os.environ.get("ILQG_DEVICE_ORDINAL", "0"))
    name = args.object
    guard = StdoutGuard()
    if name in ("config5", "config5_stored", "config5_pair"):
        variant = {"config5": "factored", "config5_stored": "stored", "config5_pair": "pair"}[name]
        o = config5(ilqg, synth, local, K=args.steps, W=args.warmup, with_cpu=not args.no_cpu_baseline, variant=variant)
    elif name == "config2":
        o = config2(ilqg, synth, local, K=args.steps, W=args.warmup)
    elif name == "dropin_b1":
        o = dropin_b1(ilqg, synth)
    elif name in ("alone", "unfused"):
        B, n_hor = args.batch or 65536, args.n_hor or 500
        x0, u0 = synth.car_batch(B, n_hor)
        t = kernel_alone(ilqg, "carparking", 0, B, n_hor, ilqg.CAR_PARAMS, x0, u0, local, args.steps,
                         **with_split(dict(fuse_derivs=1 if name == "alone" else 0), args))
        o = {k: [v[0], v[1]] for k, v in t.items()}
    else:
        raise SystemExit("bench.py: unknown --object %r" % name)
    guard.emit(json.dumps(o))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=None,
                    help="timed iterations (default 20; 3 for --config5-variant and the config5 objects, 2 for config5_stored / config5_pair)")
    ap.add_argument("--warmup", type=int, default=None, help="untimed iterations before the window (default 2; 1 for config 5)")
    ap.add_argument("--dump-outputs", default=None, metavar="DIR",
                    help="after the timed window, write what it computed to DIR/<name>.npy (dump_outputs(); at most 64 MB)")
    ap.add_argument("--config5-variant", choices=("factored", "stored", "pair"), default=None,
                    help="only BASELINE config 5 in one of its forms (the object `config5` of the --full line), as its own JSON line")
    ap.add_argument("--workload", choices=("car", "synth"), default="car",
                    help="car: BASELINE metric (CarParking n=4,m=2,N=500, 65 536 per GPU); synth: BASELINE config 5 "
                         "(n=16,m=8,N=1000, FULL_DDP=1, 16 384 per GPU, one wavefront per trajectory) as the headline")
    ap.add_argument("--batch", type=int, default=None, help="trajectories per GPU")
    ap.add_argument("--n-hor", type=int, default=None)
    ap.add_argument("--full-ddp", type=int, default=None)
    ap.add_argument("--mapping", choices=("auto", "wave"), default="auto",
                    help="wave: CarParking in the one-wavefront-per-trajectory build (comparison)")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="--full, --object config5: without the CPU baseline")
    ap.add_argument("--resweep", type=int, default=-1, help="-1: library default (off without multipliers)")
    ap.add_argument("--fuse-derivs", type=int, default=1)
    ap.add_argument("--ls-split", type=int, default=None, help="default: the library's (4; 1 in the wave mapping)")
    ap.add_argument("--bw-split", type=int, default=0, help="1: fused backward pass on two wavefronts per 64 trajectories (measured: no gain)")
    ap.add_argument("--ls-keep", type=int, default=None,
                    help="default: the library's (2 in the lane mapping: every roll-out kept, the accepted one relocated; 1 in the wave "
                         "mapping: second stage beside the re-rolled winners); 0: second stage, then winner pass")
    ap.add_argument("--no-unfused", action="store_true",
                    help="--full: skip the secondary runs (live traffic, kernels alone, full solves, config 5, config 2, drop-in)")
    ap.add_argument("--no-config5", action="store_true", help="--full: skip the config 5 objects")
    ap.add_argument("--no-live-traffic", action="store_true",
                    help="--full: do not collect the PMC traffic of the headline's kernels in this run (two short rocprofv3 child "
                         "runs); the committed, source-stamped profiles/traffic.json is quoted instead, as in a plain run")
    ap.add_argument("--solve", action="store_true",
                    help="full solves instead of the benchmark window: --batch CarParking starts solved to convergence (max_iter "
                         "--max-iter), with and without retiring finished trajectories; prints its own JSON line")
    ap.add_argument("--solve-one", type=int, default=None, help="(used by --solve) ONE full solve in this process with this `compact` setting")
    ap.add_argument("--solve-stream", type=int, default=None, help="(used by --solve) that many starts streamed through --batch resident slots, in this process")
    ap.add_argument("--max-iter", type=int, default=500)
    ap.add_argument("--compact", type=int, default=2048, help="--solve: smallest live set still gathered into a smaller context")
    ap.add_argument("--single-process", action="store_true",
                    help="--gpus N > 1 without torch.distributed.run: ONE process drives the N GPUs through the C "
                         "interface ilqg_multi_* (hipSetDevice per shard, ncclCommInitAll, one ncclGather of the costs)")
    ap.add_argument("--devices", default=None, help="--single-process: device id of every shard, e.g. 0,0,0,0,0,0,0,0")
    ap.add_argument("--backend", choices=("nccl", "gloo"), default="nccl",
                    help="torch.distributed backend of the one-process-per-GPU path; gloo: the collective's tensors go "
                         "through host memory (rehearsals on boxes with fewer GPUs than ranks, CPU tests)")
    ap.add_argument("--all-on-device", type=int, default=None, help="every rank uses this device (rehearsal of N ranks on one GPU)")
    ap.add_argument("--rehearse-protocol", action="store_true",
                    help="no solver, no GPU: the ranks run the sharding / barrier / gather / JSON protocol around a stand-in "
                         "(ProtocolShard); the line is marked `rehearsal` and measures nothing")
    ap.add_argument("--object", default=None,
                    help="(used by --full) ONE secondary object of the report — config5, config5_stored, config5_pair, "
                         "config2, dropin_b1, alone, unfused — measured in this fresh process, as one JSON line")
    ap.add_argument("--full", action="store_true",
                    help="after the headline, everything that takes runs of its own: the CPU baseline and, for the CarParking "
                         "headline on one GPU, the live PMC traffic, config 5 / its stored form / config 2 / the drop-in, the "
                         "dominant kernel alone, the two kernels of the unfused path, full solves to convergence (plain / "
                         "compacted / streamed); a plain run measures the headline alone")
    ap.add_argument("--groups", type=int, default=0,
                    help="independent sets of trajectories advanced on separate HIP streams (0: library default)")
    args = ap.parse_args()
    config5_only = args.config5_variant or (args.object or "").startswith("config5")
    if args.steps is None:
        args.steps = (2 if (args.object or "config5") != "config5" else 3) if config5_only else 20
    if args.warmup is None:
        args.warmup = 1 if config5_only else 2
    if args.steps < 1 or args.warmup < 0:
        ap.error("--steps must be at least 1 and --warmup at least 0")
    if args.dump_outputs and (args.object or args.config5_variant or args.solve or args.solve_one is not None or args.solve_stream is not None
                              or args.rehearse_protocol):
        ap.error("--dump-outputs goes with the benchmark window of the solver (the default run or --single-process)")
    if args.object:  # a child of a --full run: no torch, no process group
        return child_object(args)

    import torch
    import torch.distributed as dist
    import __graft_entry__ as g
    pkg = g.load_package()
    from ddp_generator_amd import ilqg, synth
    guard = StdoutGuard()

    rank, local, world = pkg.dist.env_world()
    if args.single_process and world == 1 and args.gpus > 1:
        return single_process(args, ilqg, synth, guard)
    if args.config5_variant:
        guard.emit(json.dumps(config5(ilqg, synth, local, K=args.steps, W=min(args.warmup, 1), with_cpu=False, variant=args.config5_variant)))
        return
    if args.solve_stream is not None:
        local = int(os.environ.get("ILQG_DEVICE_ORDINAL", local))
        guard.emit(json.dumps(solve_stream_once(ilqg, synth, local, args.batch or 65536, args.n_hor or 500, args.max_iter, args.solve_stream)))
        return
    if args.solve_one is not None:
        local = int(os.environ.get("ILQG_DEVICE_ORDINAL", local))
        guard.emit(json.dumps(solve_once(ilqg, synth, local, args.batch or 65536, args.n_hor or 500, args.max_iter, args.solve_one)))
        return
    if args.solve:
        assert world == 1 and args.workload == "car", "--solve: one GPU, CarParking"
        guard.emit(json.dumps(full_solve(local, B=args.batch or 65536, n_hor=args.n_hor or 500, max_iter=args.max_iter, compact=args.compact)))
        return
    rehearsal = args.rehearse_protocol
    if rehearsal:
        args.no_unfused = args.no_cpu_baseline = True  # (nothing of the product runs)
    if args.all_on_device is not None:
        local = args.all_on_device
    device_note = None
    if not rehearsal:
        # LOCAL_RANK is the device ordinal only while the rank sees all GPUs of the node; a launcher that narrows
        # HIP_VISIBLE_DEVICES / ROCR_VISIBLE_DEVICES per rank leaves ONE visible device, ordinal 0
        ndev = torch.cuda.device_count()
        if ndev == 0:
            raise SystemExit("bench.py: no GPU visible to rank %d (HIP_VISIBLE_DEVICES=%r)" % (rank, os.environ.get("HIP_VISIBLE_DEVICES")))
        if local >= ndev:
            if ndev == 1 and args.all_on_device is None:
                device_note = "LOCAL_RANK %d with one visible device: the launcher gave this rank its own GPU, ordinal 0" % local
                local = 0
            else:
                raise SystemExit("bench.py: rank %d has LOCAL_RANK / device %d but only %d device(s) are visible "
                                 "(HIP_VISIBLE_DEVICES=%r): launch one rank per visible GPU, or give every rank exactly one"
                                 % (rank, local, ndev, os.environ.get("HIP_VISIBLE_DEVICES")))
    host_collective = args.backend == "gloo" or rehearsal  # the collective's tensors live in host memory
    if world > 1:
        pkg.dist.init("gloo" if rehearsal else args.backend, rank, world, None if host_collective else torch.device("cuda", local))
    assert world == args.gpus or world == 1, "launch with torch.distributed.run --nproc-per-node %d" % args.gpus
    if not rehearsal:
        torch.cuda.set_device(local)
    dev = torch.device("cpu") if rehearsal else torch.device("cuda", local)
    cdev = torch.device("cpu") if host_collective else dev
    device_sync = (lambda: None) if rehearsal else torch.cuda.synchronize

    car = args.workload == "car"
    problem = "carparking" if car else "synth16x8"
    fd = args.full_ddp if args.full_ddp is not None else (0 if car else 1)
    B = args.batch if args.batch is not None else (65536 if car else 16384)
    n_hor = args.n_hor if args.n_hor is not None else (500 if car else 1000)
    K, W = args.steps, args.warmup
    nx, nu = (4, 2) if car else (16, 8)
    alg = algorithmic_bytes(nx, nu, fd)
    first = pkg.dist.shard_first(rank, B)
    x0, u0 = synth.car_batch(B, n_hor, first=first) if car else synth.synth16_batch(B, n_hor, first=first)
    params = ilqg.CAR_PARAMS if car else synth.SYNTH16_PARAMS
    if rehearsal:
        s = ProtocolShard(B, first)
    else:
        s = ilqg.BatchSolver(problem, fd, batch=B, n_hor=n_hor, device=local, params=params,
                             opts=with_split(dict(max_iter=max(K, W) + 1, fuse_derivs=args.fuse_derivs, **({"ls_keep": args.ls_keep} if args.ls_keep is not None else {}), **({"bw_split": 1} if args.bw_split else {})), args),
                             strict=("wave" if args.mapping == "wave" else False), groups=args.groups)
    if args.resweep >= 0:
        s.set_option("resweep", args.resweep)
    s.init(x0, u0)
    if W > 0:
        s.iterate(W)
        s.sync()
        s.init(x0, u0)  # back to iteration 0: the timed window is always iterations 1..K
    # device buffer the solver's per-trajectory costs are copied into (device to device) for the collective
    cost_dev = torch.empty(B, dtype=torch.float64, device=dev)

    def barrier():
        pkg.dist.barrier(world, device_sync)

    s.timing(True)  # (events come from a pool filled here: none is created inside the window)
    barrier()
    t0 = time.perf_counter()
    s.iterate(K)
    if rehearsal:
        cost_dev.copy_(torch.from_numpy(s.scalar("cost")))
    else:
        s.scalar_to_device("cost", cost_dev.data_ptr())  # synchronises the solver's streams
    # the single collective of the path: per-trajectory costs to rank 0 over RCCL/xGMI (gloo: through host memory)
    gathered = pkg.dist.gather_costs(cost_dev if cdev == dev else cost_dev.to(cdev), rank, world)
    barrier()
    dt = time.perf_counter() - t0
    dt = pkg.dist.max_over_ranks(dt, world, cdev)  # MAX over ranks

    times = s.kernel_times()
    active = s.active()
    stream_groups = s.groups()
    wave_mapping = s.problem.wave_mapping
    cost = gathered.cpu().numpy() if world > 1 and rank == 0 else s.scalar("cost")
    sweeps = None if rehearsal else float(s.ints("bp_calls").mean())  # backward sweeps (lambda retries) per trajectory, last iteration
    if args.dump_outputs and rank == 0:  # (rank 0's shard of the job: trajectories 0..B-1)
        dump_outputs(args.dump_outputs, dict({k: s.scalar(k) for k in ("cost", "lambda")}, **{k: s.ints(k) for k in ("status", "iterations")}),
                     s.x, s.u)
    s.close()

    if rank == 0:
        per_iter = {k: v[1] / max(1, K) for k, v in times.items() if v[0]}
        iter_bytes = alg["iteration"] * n_hor * B
        out = {
            "metric": ("iLQG iterations/sec, 65k-batch CarParking (n=4,m=2,N=500)" if car else
                       "iLQG iterations/sec, batch %d synthetic problem (n=16,m=8,N=%d, FULL_DDP=%d)" % (B, n_hor, fd)),
            # whole job: every rank advances its own 65 536-trajectory shard by K iterations (weak scaling), so the
            # job does world x K batch-iterations in the slowest rank's time
            "value": None if rehearsal else pkg.dist.whole_job_rate(K, dt, world),
            "unit": "iterations/s",
            "value_definition": "iterations of a %d-trajectory batch per second, whole job: %d rank(s) x %d iterations / time of "
                                "the slowest rank" % (B, world, K),
            "per_gpu_iterations_per_s": None if rehearsal else K / dt,
            "n_gpus": world,
            "steps": K,
            "warmup": W,
            "ms_per_step": 1e3 * dt / K,
            "higher_is_better": True,
            "scaling": "weak",
            "vs_baseline": None,
            "dtype": "f64",
            "data": "synthetic",
            **({"rehearsal": "protocol only (--rehearse-protocol): no solver ran, `value` is not a measurement; the costs "
                             "gathered are the trajectories' global indices", "gathered_costs_in_order":
                             bool(np.array_equal(np.floor(cost), np.arange(B * world)))} if rehearsal else {}),
            "collective": {"backend": "gloo" if rehearsal else args.backend, "tensors": "host memory" if host_collective else "device memory",
                           "doubles_per_rank": B, "gathered_on_rank_0": int(cost.size)},
            "config": {"workload": "%s batch=%d per GPU x %d GPU, 8-alpha line search, FULL_DDP=%d, "
                                   "first %d iterations after the initial roll-out" % ("CarParking" if car else "Synth16x8", B, world, fd, K),
                       "batch_per_gpu": B, "n_hor": n_hor, "n_x": nx, "n_u": nu, "full_ddp": fd,
                       "mapping": ("wave mapping (16 lanes per trajectory in the backward step where the problem allows, else one wavefront)" if wave_mapping else
                                   "one lane per trajectory (64 trajectories per wavefront)"),
                       "backward_sweeps_per_trajectory_in_last_iteration": sweeps,
                       "fuse_derivs": args.fuse_derivs, "ls_split": args.ls_split if args.ls_split is not None else "library default (4; 1 in the wave mapping)", "ls_keep": args.ls_keep if args.ls_keep is not None else "library default (2: roll-outs kept, accepted one relocated; 1 in the wave mapping)", "bw_split": args.bw_split, "resweep": args.resweep,
                       "stream_groups": stream_groups, "device_ordinal_of_rank_0": local,
                       # switches of the environment the library reads when a context is made (comparison runs): none in a default run
                       "env_switches": {k: v for k, v in sorted(os.environ.items()) if k.startswith("ILQG_") or k == "GPU_MAX_HW_QUEUES"},
                       **({"device_note": device_note} if device_note else {}),
                       "parallelism": "batch sharded over %d GPU, one RCCL gather of costs" % world},
            # PRIMARY: the whole iteration against the HBM roofline, algorithmic bytes of SURVEY 8(d)
            "iteration_roofline": {"bound": "hbm", "algorithmic_bytes_per_iteration": iter_bytes,
                                   "achieved_GBs": iter_bytes * (K / dt) / world / 1e9, "peak_GBs": HBM_PEAK_GBS,
                                   "frac_of_peak": iter_bytes * (K / dt) / world / 1e9 / HBM_PEAK_GBS,
                                   "note": "1 200 B per step and trajectory for CarParking (derivatives 488 + backward pass "
                                           "536 + line search 176): what the iteration would move with every stage's "
                                           "arrays materialised in HBM; the fused kernels move less (roofline.traffic)"},
            "kernels_ms_per_iteration_overlapping": per_iter,
            "trajectories_still_active": int(active),
            "cost_mean_after_window": float(cost.mean()),
        }
        # --full: the objects that take runs of their own (child processes, profiler passes, the host's cores); a plain
        # run reports the timed window alone
        secondary = args.full and world == 1 and not args.no_unfused and not wave_mapping and car
        if not rehearsal and not wave_mapping and car:  # (at N > 1: rank 0's own launches, its shard of the batch)
            # The two dominant launches IN THE TIMED WINDOW (HIP events on the solver's streams around every launch of the
            # K timed iterations; the groups of trajectories overlap, a launch covers one group):
            #   hbm_equivalent  SURVEY 8(d)'s algorithmic bytes of the stages the launch replaces / its duration (the
            #                   judge's recipe; NOT a utilisation: the fused kernel never moves those bytes)
            #   pmc             HBM bytes per launch from the committed rocprofv3 PMC passes (profiles/traffic.json:
            #                   FETCH_SIZE x2 + WRITE_SIZE, separate passes, gfx950 correction) / the same duration:
            #                   the real HBM utilisation
            #   valu_fp64       the reference's back_pass arithmetic / duration against the fp64 vector peak
            tj, traffic_stale = stamped("traffic.json")
            if tj is None or B != 65536:
                tj = {}
                traffic_stale = traffic_stale or "profiles/traffic.json is for 65 536 trajectories per GPU"
            traffic_source = ("profiles/traffic.json (rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE passes of this command, tools/collect_traffic.sh; "
                              "per launch of one of the stream groups; sources %s; not collected in this run)" % tj.get("_source_sha"))
            committed = dict(tj)
            if secondary and not args.no_live_traffic and B == 65536:
                live, how = live_traffic([])
                if live:
                    tj, traffic_stale, traffic_source = live, None, how
                else:
                    traffic_source += "; live collection failed: " + str(how)
            per_launch = B / max(1, stream_groups)

            def launch_object(name, alg_bytes_per_step, flops_per_step, moved_per_step):
                n_launch, total_ms = times.get(name, (0, 0.0))
                if not n_launch:
                    return None
                avg_ms = total_ms / n_launch
                o = {"kernel": name, "window": "the %d timed iterations of `value` (%d launches, %d stream groups "
                                               "overlapping, %.0f trajectories per launch)" % (K, n_launch, stream_groups, per_launch),
                     "avg_launch_ms": avg_ms, "launches": n_launch, "trajectories_per_launch": per_launch,
                     "hbm_equivalent": {"algorithmic_bytes_per_launch": alg_bytes_per_step * n_hor * per_launch,
                                        "GBs": alg_bytes_per_step * n_hor * per_launch / (avg_ms * 1e-3) / 1e9,
                                        "frac_of_peak": alg_bytes_per_step * n_hor * per_launch / (avg_ms * 1e-3) / 1e9 / HBM_PEAK_GBS},
                     "moved_bytes_per_launch_by_construction": moved_per_step * n_hor * per_launch}
                if name in tj:
                    pmc = tj[name]["hbm_bytes_per_launch"]
                    o["pmc"] = {"hbm_bytes_per_launch": pmc, "GBs": pmc / (avg_ms * 1e-3) / 1e9,
                                "frac_of_peak": pmc / (avg_ms * 1e-3) / 1e9 / HBM_PEAK_GBS,
                                "source": traffic_source}
                    if name in committed and committed is not tj:
                        o["pmc"]["committed_profile_bytes_per_launch"] = committed[name]["hbm_bytes_per_launch"]
                elif traffic_stale:
                    o["pmc"] = {"hbm_bytes_per_launch": None, "stale": traffic_stale}
                if flops_per_step:
                    o["valu_fp64"] = {"algorithmic_flops_per_launch": flops_per_step * n_hor * per_launch,
                                      "TFLOPs": flops_per_step * n_hor * per_launch / (avg_ms * 1e-3) / 1e12,
                                      "frac_of_peak": flops_per_step * n_hor * per_launch / (avg_ms * 1e-3) / 1e12 / FP64_PEAK_TFLOPS}
                return o

            bw = launch_object("k_backward[fused derivs]", alg["k_derivs"] + alg["k_backward"], backpass_flops(nx, nu, fd),
                               (nx + nu) * 8 + (nx + 2 * nu + nx * nu) * 8)
            # first stage of the line search: k_search (ls_keep = 2: every roll-out kept: + 4 x 48 B written per step) or
            # the legacy rows of k_rollout
            st1 = (launch_object("k_search[stage 1]", alg["k_rollout[search]"], 0, (nx + 2 * nu + nx * nu) * 8 + 4 * (nx + nu) * 8)
                   or launch_object("k_rollout[search]", alg["k_rollout[search]"], 0, (nx + 2 * nu + nx * nu) * 8))
            if bw:
                out["roofline"] = {
                    # bound / achieved / peak / unit / frac: the contract's HBM figure (algorithmic bytes over the launch's
                    # duration against 8 TB/s).  What limits the kernel is in `limiter` / `issue`.
                    "bound": "hbm", "kernel": bw["kernel"],
                    "achieved": bw["hbm_equivalent"]["GBs"], "peak": HBM_PEAK_GBS, "unit": "GB/s",
                    "frac": bw["hbm_equivalent"]["frac_of_peak"],
                    "traffic": bw.get("pmc", {}).get("hbm_bytes_per_launch"),
                    "frac_kind": "hbm_equivalent: ALGORITHMIC bytes of the launch / its duration / peak (the contract's recipe); "
                                 "the launch's real HBM utilisation is hbm_utilisation_frac",
                    "hbm_utilisation_frac": bw.get("pmc", {}).get("frac_of_peak"),
                    "limiter": "valu_issue (fp64 vector instruction issue of ONE wavefront per SIMD, and the divergence of the box QP)",
                    "issue": issue_object("k_backward<2>"),
                    "dominant_launch": bw, "second_launch": st1,
                    "note": "achieved / frac follow the contract's recipe: SURVEY 8(d)'s ALGORITHMIC bytes of the launch "
                            "(the 1 024 B per step and trajectory of the two stages this kernel replaces x steps x the "
                            "trajectories of one launch) over its average duration in the timed window.  It is an "
                            "HBM-EQUIVALENT rate, not a utilisation: the kernel evaluates the derivatives of a step in "
                            "registers and moves 176 B per step (`traffic`, PMC: dominant_launch.pmc is its real HBM "
                            "utilisation).  What bounds it is fp64 vector issue and the divergence of the box QP: "
                            "dominant_launch.valu_fp64 prices the reference's back_pass arithmetic (%d flop per step and "
                            "trajectory, backpass_flops(); the derivative callbacks it also evaluates are not counted) — "
                            "one of %d launches that share the chip in the window; `alone` = the same kernel with the batch "
                            "as ONE group and nothing else on the GPU, over the same %d iterations."
                            % (backpass_flops(nx, nu, fd), stream_groups, K)}
        if secondary:
            # Every secondary object is measured in a fresh child process (run_object): its own HIP context and queues,
            # its buffers allocated into an empty device — this process has released the solver and holds only torch's
            # context.  A failure is reported in place and never costs the headline.
            # the dominant kernel ALONE: one group of trajectories, so a launch covers the whole batch and shares the
            # GPU with nothing; the SAME K iterations as the headline window (the kernel grows with the iterations)
            t1 = run_object("alone", local, ["--steps", K, "--batch", B, "--n-hor", n_hor] + (["--ls-split", args.ls_split] if args.ls_split is not None else []))
            name = "k_backward[fused derivs]"
            if "error" not in t1 and t1.get(name, [0])[0] and "roofline" in out:
                n_launch, total_ms = t1[name]
                avg_ms = total_ms / n_launch
                flops_launch = backpass_flops(nx, nu, fd) * n_hor * B
                out["roofline"]["alone"] = {
                    "avg_launch_ms": avg_ms, "launches": n_launch, "stream_groups": 1, "trajectories_per_launch": B,
                    "valu_fp64_TFLOPs": flops_launch / (avg_ms * 1e-3) / 1e12,
                    "valu_fp64_frac": flops_launch / (avg_ms * 1e-3) / 1e12 / FP64_PEAK_TFLOPS,
                    "hbm_equivalent_GBs": (alg["k_derivs"] + alg["k_backward"]) * n_hor * B / (avg_ms * 1e-3) / 1e9,
                    "note": "one wavefront per SIMD (65 536 lanes): a chain of dependent fp64 instructions, see DESIGN.md; "
                            "hbm_equivalent above the 8 TB/s peak means the fused kernel beats what the unfused pair could reach"}
                out["kernels_ms_per_iteration_alone"] = {k: v[1] / K for k, v in t1.items() if v[0]}
            elif "error" in t1:
                out["kernels_ms_per_iteration_alone"] = t1
            # the HBM-bound kernels of the unfused path, each alone
            t2 = run_object("unfused", local, ["--steps", 5, "--batch", B, "--n-hor", n_hor] + (["--ls-split", args.ls_split] if args.ls_split is not None else []))
            unfused = {}
            for kname in ("k_derivs", "k_backward"):
                n, ms = t2.get(kname, (0, 0.0)) if "error" not in t2 else (0, 0.0)
                if n:
                    b_alg = alg[kname] * n_hor * B
                    unfused[kname] = {"bound": "hbm", "avg_launch_ms": ms / n, "algorithmic_bytes_per_launch": b_alg,
                                      "achieved_GBs": b_alg / (ms / n * 1e-3) / 1e9,
                                      "frac_of_peak": b_alg / (ms / n * 1e-3) / 1e9 / HBM_PEAK_GBS, "stream_groups": 1}
            out["unfused_kernels"] = unfused if "error" not in t2 else t2
            try:
                out["full_solve"] = full_solve(local)
            except Exception as e:
                out["full_solve"] = {"error": "%s: %s" % (type(e).__name__, e)}
            out["dropin_b1"] = run_object("dropin_b1", local)
            out["config2"] = run_object("config2", local, ["--steps", 20, "--warmup", 2])
            if not args.no_config5:
                out["config5"] = run_object("config5", local, ["--steps", 3, "--warmup", 1] + (["--no-cpu-baseline"] if args.no_cpu_baseline else []))
                out["config5_stored"] = run_object("config5_stored", local, ["--steps", 2, "--warmup", 1, "--no-cpu-baseline"])
        elif not car:
            flops = backpass_flops(nx, nu, fd) * n_hor * B
            out["roofline"] = {"bound": "hbm", "kernel": "iteration", "achieved": iter_bytes * (K / dt) / world / 1e9,
                               "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": iter_bytes * (K / dt) / world / 1e9 / HBM_PEAK_GBS,
                               "traffic": None, "backward_fp64_frac": flops * (K / dt) / world / 1e12 / FP64_PEAK_TFLOPS}
        if "roofline" not in out:  # the protocol rehearsal, or kernel timing unavailable: the iteration-level figure
            out["roofline"] = {"bound": "hbm", "kernel": "iteration", "achieved": out["iteration_roofline"]["achieved_GBs"],
                               "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": out["iteration_roofline"]["frac_of_peak"],
                               "traffic": None, "note": "per GPU; algorithmic bytes of SURVEY 8(d) per iteration x "
                                                        "iterations/s."}
        if args.full and not args.no_cpu_baseline:  # rank 0, whatever the world size: the host's cores are the same
            out["cpu_baseline"] = cpu_baseline(B, K, problem, fd, params, n_hor,
                                               synth.car_batch if car else synth.synth16_batch)
        guard.emit(compact_line(out, write_detail(out)))
    if world > 1:
        dist.barrier()  # (rank 0 may still have been timing the CPU baseline)
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
