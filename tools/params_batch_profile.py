#!/usr/bin/env python3
"""What problem parameters per trajectory cost the planner (BatchSolver.set_params_batch, the instantiations of the lane-mapped
kernels that take the context's table) at BASELINE config 3.

    python tools/params_batch_profile.py [--repeats 10] [--steps 20] [--warmup 5] [--batch 65536] [--timed 3]

One process.  The window is bench.py's own: 65 536 CarParking trajectories (synth.car_batch), init, `--warmup` iterations,
init again, then `--steps` iterations and the read of the costs between two host clock readings.  Two legs ALTERNATE,
`--repeats` times, on ONE solver (its buffers, stream groups and roll-out planes are the same for both):
  (a) the shared batch — no per-trajectory set: the kernels every batch ran before there was one;
  (b) the same batch with a NOMINAL table of all fixed-size parameters (every row holds the batch's own values, so both legs
      walk the same trajectories): what the vector registers that hold the rows cost.
Printed: iterations/s of every repeat, medians and ranges, the ratio of the medians (b) / (a), and — from `--timed` further
alternations with per-kernel timing on — the HIP-event time per launch of every kernel in both legs.  (a) is to be read against `python bench.py` of the parent commit on the same box and that
box's run-to-run band (profiles/r6_bench_default_runs.txt).  Not part of bench.py.

    python tools/params_batch_profile.py --step-rows [--repeats 10] [--steps 20] [--warmup 5] [--batch 65536] [--timed 3]

The per-time-step leg (`--steps` is the iteration count above, hence the other name): almix FULL_DDP = 1, N = 80, the same
window and alternation.  (a) is the shared window of `vref`; (b) the same batch with NOMINAL rows of `vref`
(BatchSolver.set_param_steps_batch): what a window per lane — a pointer in two vector registers, a vector load per use where
the shared window takes a scalar one — costs.  Then k_shift_param_rows per launch (shift_param_batch by 1 with a tail)
against re-sending the moved rows through the host setter, host wall time per call, `--repeats` alternations.
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def spread(v, unit):
    v = np.asarray(v, dtype=np.float64)
    return "median %9.3f %s  min %9.3f  max %9.3f  (n = %d)" % (np.median(v), unit, v.min(), v.max(), len(v))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--batch", type=int, default=65536)
    ap.add_argument("--timed", type=int, default=3, help="further alternations with per-kernel HIP-event timing, behind the rate repeats")
    ap.add_argument("--step-rows", action="store_true", help="the per-time-step leg: almix, nominal rows of vref against the shared window")
    a = ap.parse_args()
    import __graft_entry__ as g
    g.load_package()
    from ddp_generator_amd import ilqg, synth
    B, K, W = a.batch, a.steps, a.warmup
    if a.step_rows:
        from oracle.harness import almix_case
        params, opts, x0, u0 = almix_case(batch=B)
        N = u0.shape[1]
        s = ilqg.BatchSolver("almix", 1, batch=B, n_hor=N, params=params, opts=dict(opts, max_iter=max(K, W) + 1))
        rows = np.ascontiguousarray(np.tile(np.asarray(params["vref"], dtype=np.float64), (B, 1)))
        print("== almix FULL_DDP=1, %d trajectories, N = %d, %d stream group(s); %d warm-up + %d timed iterations, %d alternating repeats"
              % (B, N, s.groups(), W, K, a.repeats))
        print("   (b): nominal rows of vref, [%d][%d], every row the shared window" % rows.shape, flush=True)

        def set_leg(per_trajectory):
            s.set_param_steps_batch("vref", rows if per_trajectory else None)
    else:
        N = 500
        x0, u0 = synth.car_batch(B, N)
        s = ilqg.BatchSolver("carparking", 0, batch=B, n_hor=N, params=ilqg.CAR_PARAMS, opts=dict(max_iter=max(K, W) + 1))
        fixed = [(n, size) for n, size in s.problem.params if size > 0]
        table = {n: np.ascontiguousarray(np.broadcast_to(np.asarray(ilqg.CAR_PARAMS[n], dtype=np.float64).reshape(-1), (B, size))) for n, size in fixed}
        print("== config 3: carparking FULL_DDP=0, %d trajectories, N = %d, %d stream group(s); %d warm-up + %d timed iterations, %d alternating repeats"
              % (B, N, s.groups(), W, K, a.repeats))
        print("   (b): %d fixed-size parameters named, %d doubles per row (%s), every row the batch's own values" % (
            len(fixed), sum(size for _, size in fixed), ", ".join(n for n, _ in fixed)), flush=True)

        def set_leg(per_trajectory):
            s.set_params_batch(table if per_trajectory else {})

    def window(per_trajectory):
        set_leg(per_trajectory)
        s.init(x0, u0)
        if W > 0:
            s.iterate(W)
            s.sync()
            s.init(x0, u0)
        s.sync()
        t0 = time.perf_counter()
        s.iterate(K)
        cost = s.scalar("cost")  # (synchronises)
        s.sync()
        return K / (time.perf_counter() - t0), cost

    for leg in (False, True):  # once untimed: buffers, roll-out planes, the table
        window(leg)
    rate = {False: [], True: []}
    kern = {False: {}, True: {}}
    costs = {}
    for r in range(a.repeats):  # the rates: per-kernel timing off, as in bench.py
        for leg in (False, True):
            v, costs[leg] = window(leg)
            rate[leg].append(v)
            print("   repeat %2d %s: %8.2f iterations/s" % (r, "(b) per-trajectory" if leg else "(a) shared        ", v), flush=True)
    s.timing(True)
    for r in range(a.timed):  # the kernels: the same alternation with HIP events around every launch
        for leg in (False, True):
            k0 = s.kernel_times()
            window(leg)
            k1 = s.kernel_times()
            for name in k1:
                n = k1[name][0] - k0.get(name, (0, 0.0))[0]
                if n > 0:
                    kern[leg].setdefault(name, []).append((k1[name][1] - k0.get(name, (0, 0.0))[1]) / n)
    s.timing(False)
    print("(a) shared batch:              " + spread(rate[False], "it/s"))
    print("(b) nominal table of all rows: " + spread(rate[True], "it/s"))
    ma, mb = np.median(rate[False]), np.median(rate[True])
    print("ratio of medians (b) / (a): %.3f  ((a)'s repeats span %.3f .. %.3f of its median, (b)'s %.3f .. %.3f of its)" % (
        mb / ma, np.min(rate[False]) / ma, np.max(rate[False]) / ma, np.min(rate[True]) / mb, np.max(rate[True]) / mb))
    print("costs of the two legs: worst relative difference %.3g (the same trajectories in other kernels)" % float(
        np.max(np.abs(costs[True] - costs[False]) / np.maximum(1.0, np.abs(costs[False])))))
    print("HIP-event time per launch, medians over %d further alternations with per-kernel timing on (warm-up launches included):" % a.timed)
    for name in sorted(kern[False]):
        if name in kern[True]:
            ta, tb = np.median(kern[False][name]), np.median(kern[True][name])
            print("   %-22s (a) %8.4f ms   (b) %8.4f ms   (b) / (a) %.3f" % (name, ta, tb, tb / ta if ta > 0 else float("nan")))
    if a.step_rows:  # the window shift in place against re-sending the moved rows through the host setter
        s.set_param_steps_batch("vref", rows)
        tail = np.ascontiguousarray(rows[:, -1:])
        moved = np.ascontiguousarray(np.concatenate([rows[:, 1:], tail], axis=1))
        t_shift, t_send = [], []
        s.timing(True)
        k0 = s.kernel_times()["k_shift_param_rows"]
        for r in range(a.repeats):
            s.sync()
            t0 = time.perf_counter()
            s.shift_param_batch("vref", 1, tail)
            s.sync()
            t_shift.append(1e3 * (time.perf_counter() - t0))
            t0 = time.perf_counter()
            s.set_param_steps_batch("vref", moved)
            s.sync()
            t_send.append(1e3 * (time.perf_counter() - t0))
        k1 = s.kernel_times()["k_shift_param_rows"]
        print("shift_param_batch(1, tail), host wall time per call:   " + spread(t_shift, "ms"))
        print("set_param_steps_batch of the moved rows, per call:     " + spread(t_send, "ms"))
        print("k_shift_param_rows, HIP-event time per launch: %.4f ms (%d launches, one per stream group and call)" % (
            (k1[1] - k0[1]) / max(k1[0] - k0[0], 1), k1[0] - k0[0]))
    s.close()


if __name__ == "__main__":
    main()
