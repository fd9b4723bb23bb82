#!/usr/bin/env python3
"""Multi-start between two control intervals: pick each agent's best plan and start all its candidates from it, on the device
(BatchSolver.best_of + shift_winners) against the same interval through the host, and against the plain shift.

    python tools/best_of_profile.py [--agents 8192] [--candidates 8] [--repeats 10] [--steps 1] [--warmup 20] [--between 2]

CarParking FULL_DDP 0 at n_hor = 500 (BASELINE config 3) as `--agents` agents x `--candidates` candidates.  One process.  After
`--warmup` iterations three forms of the step behind iterate ALTERNATE, `--between` solver iterations in front of each, so that
every one finds the batch as a control loop would (current trajectories in the kept roll-out planes of the line search):
    (a) device   best_of(device=True) + shift_winners with CUDA tensors: winners never leave the GPU, du is a tensor that is
                 already there (a fresh perturbation per round is the caller's; its generation is not timed)
    (b) host     the parent's means: scalar("cost"), ints("status"), x(), u(), the numpy rule, init(x0', u')
    (c) shift    plain shift(steps): one plan per slot, the parent's entry and the yardstick
Each is timed by the host clock between two device synchronisations; the new kernels' own times are HIP events
(ilqg_batch_get_timing).  Not part of bench.py.
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--agents", type=int, default=8192)
    ap.add_argument("--candidates", type=int, default=8)
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--steps", type=int, default=1)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--between", type=int, default=2)
    a = ap.parse_args()
    import __graft_entry__ as g
    g.load_package()
    from ddp_generator_amd import ilqg, synth

    K, G, N, steps = a.candidates, a.agents, 500, a.steps
    B = G * K
    x0, u0 = synth.car_batch(B, N)
    s = ilqg.BatchSolver("carparking", 0, batch=B, n_hor=N, params=ilqg.CAR_PARAMS, opts=dict(max_iter=1 << 20))
    nx, nu = s.problem.nx, s.problem.nu
    print("== CarParking FULL_DDP=0, %d agents x %d candidates = %d trajectories, N = %d, shift by %d step(s), %d stream group(s)" % (
        G, K, B, N, steps, s.groups()))
    s.init(x0, u0)
    s.iterate(a.warmup)
    s.sync()
    import torch
    rng = np.random.default_rng(3)
    du = 0.01 * rng.standard_normal((B, N, nu))
    du[::K] = 0.0
    du_dev = torch.from_numpy(du).cuda()

    def device():
        winner, _, _ = s.best_of(K, device=True)
        s.shift_winners(K, winner, steps, du=du_dev)

    def host():  # (the rule of tests/bestof_cases.py in whole-array numpy: argmin returns the first of equal minima)
        cost, status = s.scalar("cost"), s.ints("status")
        score = np.where(np.isfinite(cost) & (status != 7), cost, np.inf).reshape(G, K)
        winner = np.where(np.isfinite(score).any(axis=1), np.arange(G) * K + score.argmin(axis=1), -1)
        src = np.where(np.repeat(winner, K) >= 0, np.repeat(winner, K), np.arange(B))
        x, u = s.x(), s.u()
        s.init(x[src, steps], np.concatenate([u[src, steps:], np.repeat(u[src, -1:], steps, axis=1)], axis=1) + du)

    def shift():
        s.shift(steps)

    forms = (("device", device), ("host", host), ("shift", shift))
    for _, f in forms:  # once untimed: staging buffers, torch's allocations
        f()
        s.iterate(a.between)
    s.sync()
    s.timing(True)
    t = {name: [] for name, _ in forms}
    for r in range(a.repeats):
        for name, f in forms:
            s.iterate(a.between)
            s.sync()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            f()
            s.sync()
            torch.cuda.synchronize()
            t[name].append(1e3 * (time.perf_counter() - t0))
    kt, busy = s.kernel_times(), s.kernel_busy()
    s.timing(False)
    print("(a) best_of_device + shift_winners_device:   " + spread(t["device"]))
    print("(b) through the host (numpy rule, init):     " + spread(t["host"]))
    print("(c) plain shift:                             " + spread(t["shift"]))
    md, mh, ms_ = (np.median(t[k]) for k in ("device", "host", "shift"))
    print("medians: (a) - (c) = %.3f ms; (b) / (a) = %.1f" % (md - ms_, mh / md))
    for name in ("k_best_of", "k_shift_winners", "k_shift", "k_rollout[init]"):
        n, ms = kt[name]
        if n:
            print("%s: %d launches, %.4f ms per launch, %.3f ms of wall clock per use (union of the groups' launches)" % (
                name, n, ms / n, busy.get(name, 0.0) / a.repeats / (3 if name == "k_rollout[init]" else 1)))
    print("(a) reads du: %.2f GB per interval; (b) moves %.2f GB down and %.2f GB up" % (
        B * N * nu * 8 / 1e9, (B * (N + 1) * nx + B * N * nu) * 8 / 1e9, (B * nx + B * N * nu) * 8 / 1e9))
    s.close()


if __name__ == "__main__":
    main()
