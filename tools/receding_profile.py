#!/usr/bin/env python3
"""Receding-horizon re-plan: on the device (BatchSolver.shift) against through the host (x(), u(), a numpy shift, init()).

    python tools/receding_profile.py [--config headline|config5|both] [--repeats 10] [--steps 10] [--warmup 20]

One process per invocation.  After `--warmup` iterations the two re-plans ALTERNATE; each is timed by the host clock
between two device synchronisations, and two solver iterations run between re-plans so that every one of them finds the
batch as a control loop would (lane mapping: current trajectories in the kept roll-out planes of the line search).  The
new kernels' own times are HIP events (ilqg_batch_get_timing).  Not part of bench.py.
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def spread(v):
    v = np.asarray(v)
    return "median %9.2f ms  min %9.2f  max %9.2f  (n = %d)" % (np.median(v), v.min(), v.max(), len(v))


def run(ilqg, synth, config, repeats, steps, warmup, between):
    if config == "headline":
        problem, fd, B, N, params = "carparking", 0, 65536, 500, ilqg.CAR_PARAMS
        x0, u0 = synth.car_batch(B, N)
    else:
        problem, fd, B, N, params = "synth16x8", 1, 16384, 1000, synth.SYNTH16_PARAMS
        x0, u0 = synth.synth16_batch(B, N)
    s = ilqg.BatchSolver(problem, fd, batch=B, n_hor=N, params=params, opts=dict(max_iter=1 << 20))
    nx, nu = s.problem.nx, s.problem.nu
    print("== %s: %s FULL_DDP=%d, %d trajectories, N = %d, shift by %d steps, %d stream group(s), %s mapping" % (
        config, problem, fd, B, N, steps, s.groups(), "wave" if s.problem.wave_mapping else "lane"))
    s.init(x0, u0)
    s.iterate(warmup)
    s.sync()

    def device_replan():
        s.shift(steps)

    def host_replan():  # what a caller had to do before ilqg_batch_shift existed
        x, u = s.x(), s.u()
        s.init(x[:, steps], np.concatenate([u[:, steps:], np.repeat(u[:, -1:], steps, axis=1)], axis=1))

    for f in (device_replan, host_replan):  # once untimed: staging buffers, pinned memory
        f()
        s.iterate(between)
    s.sync()
    s.timing(True)
    t = {"device": [], "host": []}
    for r in range(repeats):
        for name, f in (("device", device_replan), ("host", host_replan)):
            s.iterate(between)
            s.sync()
            t0 = time.perf_counter()
            f()
            s.sync()
            t[name].append(1e3 * (time.perf_counter() - t0))
    kt, busy = s.kernel_times(), s.kernel_busy()
    s.timing(False)
    dev, host = np.array(t["device"]), np.array(t["host"])
    print("device re-plan (shift):                     " + spread(dev))
    print("host re-plan (x, u, numpy, init):           " + spread(host))
    print("ratio of medians host / device: %.1f; slowest device re-plan %.2f ms against fastest host re-plan %.2f ms" % (
        np.median(host) / np.median(dev), dev.max(), host.min()))
    n, ms = kt["k_shift"]
    moved = 2.0 * B * N * nu * 8  # one read and one write of U
    print("k_shift: %d launches (%d per re-plan), %.3f ms per launch, %.3f ms of wall clock per re-plan (union of the groups' launches)" % (
        n, n // repeats, ms / n, busy.get("k_shift", 0.0) / repeats))
    print("k_shift moves %.3f GB per re-plan (read + write of U, B N N_U doubles each): %.2f TB/s per launch, %.2f TB/s over the union" % (
        moved / 1e9, moved / s.groups() / (ms / n * 1e-3) / 1e12, moved / (busy["k_shift"] / repeats * 1e-3) / 1e12))
    n, ms = kt["k_rollout[init]"]
    print("k_rollout[init]: %d launches, %.3f ms per launch (device and host re-plans alike)" % (n, ms / n))
    n, ms = kt["layout kernels"]
    print("layout kernels (host re-plan's transposes): %d launches, %.3f ms in all per host re-plan" % (n, ms / repeats))
    print("through the host per re-plan: %.2f GB down, %.2f GB up" % ((B * (N + 1) * nx + B * N * nu) * 8 / 1e9, (B * nx + B * N * nu) * 8 / 1e9))
    s.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="both", choices=("headline", "config5", "both"))
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--between", type=int, default=2, help="solver iterations between two re-plans")
    a = ap.parse_args()
    import __graft_entry__ as g
    g.load_package()
    from ddp_generator_amd import ilqg, synth
    for config in (("headline", "config5") if a.config == "both" else (a.config,)):
        run(ilqg, synth, config, a.repeats, a.steps, a.warmup, a.between)


if __name__ == "__main__":
    main()
