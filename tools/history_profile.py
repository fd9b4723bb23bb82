#!/usr/bin/env python3
"""What recording the iteration history costs (BatchSolver.set_history, k_history) at BASELINE config 3.

    python tools/history_profile.py [--batch 65536] [--cap 32] [--repeats 10] [--steps 20] [--warmup 5]

One process.  Two solvers of the library's default grouping on the same CarParking starts, one with a history of `--cap`
entries and one without.  After `--warmup` iterations each, the two ALTERNATE `--repeats` times: init (which also clears the
history), `--steps` iterations between two device synchronisations on the host clock -> iterations/s.  Then one more window
of each with per-kernel HIP-event timing on: launches and time per launch of k_history beside k_update's, and the launch
counts of every kernel of the two solvers side by side.  Last, the states of the two solvers are compared bit for bit.
Not part of bench.py."""
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
    ap.add_argument("--batch", type=int, default=65536)
    ap.add_argument("--cap", type=int, default=32)
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    a = ap.parse_args()
    import __graft_entry__ as g
    pkg = g.load_package()
    from ddp_generator_amd import ilqg
    B, N = a.batch, 500
    x0, u0 = pkg.synth.car_batch(B, N)
    mk = lambda: ilqg.BatchSolver("carparking", 0, batch=B, n_hor=N, params=ilqg.CAR_PARAMS, opts=dict(max_iter=1 << 20))
    off, on = mk(), mk()
    on.set_history(a.cap)
    print("== CarParking FULL_DDP=0, %d trajectories, N = %d, %d stream groups, history of cap = %d (%.1f MB on the device) against none" % (
        B, N, on.groups(), a.cap, (7 * 8 + 3 * 4) * a.cap * B / 1e6), flush=True)

    def window(s):
        s.init(x0, u0)
        s.sync()
        t = time.perf_counter()
        s.iterate(a.steps)
        s.sync()
        return a.steps / (time.perf_counter() - t)

    for s in (off, on):
        s.init(x0, u0)
        s.iterate(a.warmup)
        s.sync()
    rate = {"off": [], "on": []}
    for r in range(a.repeats):
        for tag, s in (("off", off), ("on", on)) if r % 2 == 0 else (("on", on), ("off", off)):
            rate[tag].append(window(s))
    for tag in ("off", "on"):
        print("iterate, history %-3s: %s" % (tag, spread(rate[tag], "it/s")))
    ratio = np.median(rate["on"]) / np.median(rate["off"])
    print("median on / median off = %.4f (%+.2f %%)" % (ratio, 100 * (ratio - 1)))
    times = {}
    for tag, s in (("off", off), ("on", on)):
        s.timing(True)
        window(s)
        times[tag] = s.kernel_times()
        s.timing(False)
    for k in ("k_update", "k_history"):
        n, ms = times["on"][k]
        print("history on:  %-10s %4d launches, %8.4f ms per launch" % (k, n, ms / n if n else 0.0))
    n, ms = times["off"]["k_update"]
    print("history off: %-10s %4d launches, %8.4f ms per launch; k_history %d launches" % ("k_update", n, ms / n, times["off"]["k_history"][0]))
    differ = [k for k in times["on"] if k != "k_history" and times["on"][k][0] != times["off"][k][0]]
    print("launch counts of every other kernel equal: %s" % (not differ) + ("" if not differ else "  differ: %s" % differ))
    assert times["on"]["k_history"][0] == a.steps * on.groups() and times["off"]["k_history"][0] == 0
    same = all(np.array_equal(p, q) for p, q in ((on.x(), off.x()), (on.u(), off.u()), (on.scalar("cost"), off.scalar("cost")),
                                                 (on.scalar("lambda"), off.scalar("lambda")), (on.ints("iterations"), off.ints("iterations"))))
    print("x, u, cost, lambda, iterations of the two solvers equal bit for bit: %s" % same)
    h = on.history(("n", "alpha_idx"))
    print("recorded: n = %d .. %d; accepted step index histogram of the window (1-based, 9 = none): %s" % (
        h["n"].min(), h["n"].max(), np.bincount(h["alpha_idx"][:, :a.steps].reshape(-1), minlength=10)[1:].tolist()))


if __name__ == "__main__":
    main()
