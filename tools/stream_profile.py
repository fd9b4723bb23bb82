#!/usr/bin/env python3
"""What a stream of starts costs with trajectories, parameter rows per start and a history per start
(BatchSolver.solve_stream, ilqg_batch_solve_stream_rows; finished starts come back through k_harvest).

    python tools/stream_profile.py [--repeats 10] [--batch 32768] [--total 65536] [--max-iter 500] [--legs s,t,r,h] [--history 32]

One process, ONE solver (its buffers, stream groups and roll-out planes are the same for every leg).  `--total` CarParking
starts (synth.car_batch, the benchmark's generator) go through `--batch` resident slots, solved to the reference's exit
tests; a leg is one solve_stream between two host clock readings.  The legs ALTERNATE, `--repeats` times:
  (s) the shared stream: solve_stream(x0, u0) — cost, status and iterations per start;
  (t) with_trajectories=True: x and u of every start come back too;
  (r) rows: a NOMINAL table of all fixed-size parameters per start (every row holds the batch's own values, so the legs walk
      the same trajectories): the upload of m x W per refill and the kernels that take the context's table;
  (h) history=`--history`: every start records and brings back its iteration history.
Printed: solves/s of every repeat, medians and ranges per leg, the ratios of the medians to (s), and per leg the counts of the
last repeat (polls, launches of k_harvest, bytes they copied to the host), k_harvest's HIP-event time per launch (from one
further repeat per leg with per-kernel timing on; it is timed in the slot of the layout kernels, which a lane-mapped stream
with fused derivatives launches nothing else in) and, for (h), the bytes per poll against the read of the whole batch's
history that the harvest replaces (B x cap x 12 fields).  `--legs s,t` runs on a library built before the new entry existed
(the parent commit): (t) against (t) is the harvest kernel against a context per poll.  Not part of bench.py.
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

LEGS = {"s": "(s) shared stream       ", "t": "(t) with trajectories   ", "r": "(r) nominal rows / start", "h": "(h) history per start   "}


def spread(v, unit):
    v = np.asarray(v, dtype=np.float64)
    return "median %10.1f %s  min %10.1f  max %10.1f  (n = %d)" % (np.median(v), unit, v.min(), v.max(), len(v))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--batch", type=int, default=32768)
    ap.add_argument("--total", type=int, default=65536)
    ap.add_argument("--max-iter", type=int, default=500)
    ap.add_argument("--history", type=int, default=32)
    ap.add_argument("--legs", default="s,t,r,h")
    a = ap.parse_args()
    legs = [k for k in a.legs.split(",") if k]
    assert legs and all(k in LEGS for k in legs), "--legs: a comma-separated choice of s, t, r, h"
    import __graft_entry__ as g
    g.load_package()
    from ddp_generator_amd import ilqg, synth
    B, N, total = a.batch, 500, a.total
    x0, u0 = synth.car_batch(total, N)
    s = ilqg.BatchSolver("carparking", 0, batch=B, n_hor=N, params=ilqg.CAR_PARAMS, opts=dict(max_iter=a.max_iter))
    fixed = [(n, size) for n, size in s.problem.params if size > 0]
    table = {n: np.ascontiguousarray(np.broadcast_to(np.asarray(ilqg.CAR_PARAMS[n], dtype=np.float64).reshape(-1), (total, size))) for n, size in fixed}
    kw = {"s": {}, "t": dict(with_trajectories=True), "r": dict(params=table), "h": dict(history=a.history)}
    print("== carparking FULL_DDP=0, %d starts through %d slots, N = %d, max_iter %d, %d stream group(s); legs %s, %d alternating repeats"
          % (total, B, N, a.max_iter, s.groups(), ",".join(legs), a.repeats))
    if "r" in legs:
        print("   (r): %d fixed-size parameters named, %d doubles per row" % (len(fixed), sum(size for _, size in fixed)))
    sys.stdout.flush()

    def run(leg):
        s.sync()
        t0 = time.perf_counter()
        out = s.solve_stream(x0, u0, **kw[leg])
        s.sync()
        return total / (time.perf_counter() - t0), out

    counted = hasattr(s, "stream_counts") and hasattr(s.lib, "ilqg_batch_stream_counts")
    run(legs[0])  # once untimed: buffers, roll-out planes, the staging context's first allocation
    rate, counts, cost = {k: [] for k in legs}, {}, {}
    for r in range(a.repeats):
        for leg in legs:
            v, out = run(leg)
            rate[leg].append(v)
            cost[leg] = out["cost"]
            if counted:
                counts[leg] = s.stream_counts()
            print("   repeat %2d %s: %10.1f solves/s" % (r, LEGS[leg], v), flush=True)
    per_launch = {}
    s.timing(True)
    for leg in legs:  # the kernel: one further repeat per leg with HIP events around every launch
        k0 = s.kernel_times().get("layout kernels", (0, 0.0))
        run(leg)
        k1 = s.kernel_times().get("layout kernels", (0, 0.0))
        if k1[0] > k0[0]:
            per_launch[leg] = ((k1[1] - k0[1]) / (k1[0] - k0[0]), k1[0] - k0[0])
    s.timing(False)
    for leg in legs:
        print("%s: %s" % (LEGS[leg], spread(rate[leg], "solves/s")))
    base = np.median(rate[legs[0]])
    for leg in legs[1:]:
        m = np.median(rate[leg])
        print("ratio of medians %s / %s: %.3f  (repeats span %.3f .. %.3f of their median)" % (
            leg, legs[0], m / base, np.min(rate[leg]) / m, np.max(rate[leg]) / m))
    for leg in legs[1:]:
        print("costs of leg %s against leg %s: %s" % (leg, legs[0], "identical" if np.array_equal(cost[leg], cost[legs[0]]) else "DIFFERENT"))
    for leg in legs:
        if leg in counts:
            c = counts[leg]
            line = "%s: %d polls, %d launches of k_harvest, %.2f MB copied to the host by them (%.1f KB per poll)" % (
                LEGS[leg], c["polls"], c["harvests"], c["harvest_bytes"] / 1e6, c["harvest_bytes"] / 1e3 / max(c["polls"], 1))
            if leg in per_launch:
                line += "; k_harvest %.4f ms per launch (%d launches timed)" % per_launch[leg]
            print(line)
            if leg == "h":
                whole = B * a.history * (9 * 8 + 3 * 4)
                print("   the read of the whole batch's history it replaces: B x cap x 12 fields = %.1f MB per poll, %.0f times the harvest's"
                      % (whole / 1e6, whole / max(c["harvest_bytes"] / max(c["polls"], 1), 1.0)))
        elif leg in per_launch:
            print("%s: layout kernels %.4f ms per launch (%d launches timed)" % ((LEGS[leg],) + per_launch[leg]))
    s.close()


if __name__ == "__main__":
    main()
