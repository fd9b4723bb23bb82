#!/usr/bin/env python3
"""Receding-horizon re-plan: on the device (BatchSolver.shift) against through the host (x(), u(), a numpy shift, init()).

    python tools/receding_profile.py [--config headline|config5|both] [--repeats 10] [--steps 10] [--warmup 20]
    python tools/receding_profile.py --loop external [--config ...] [--repeats 10] [--steps 1] [--iterations 2]
    python tools/receding_profile.py --loop plant [--config ...] [--repeats 10] [--steps 1] [--iterations 2] [--rounds 5]
    python tools/receding_profile.py --loop windows [--batch 65536] [--repeats 10] [--steps 1] [--iterations 2] [--rounds 10]

One process per invocation.  After `--warmup` iterations the two re-plans ALTERNATE; each is timed by the host clock
between two device synchronisations, and two solver iterations run between re-plans so that every one of them finds the
batch as a control loop would (lane mapping: current trajectories in the kept roll-out planes of the line search).  The
new kernels' own times are HIP events (ilqg_batch_get_timing).  Not part of bench.py.

--loop external: one control interval of a caller with its OWN plant, {iterate(k); read what is applied; plant; shift with
the measured state}, in the forms a caller has — through whole fields on the host (u(), with or without x(), and a host
x_meas) and with the heads and x_meas staying on the GPU as torch tensors (head(device=True), shift(cuda tensor)).  The
plant is trivial: x_meas = x[steps] of the plan + noise (a random walk of x_meas where the form does not read x).  The
forms ALTERNATE in one process.  Per form and repeat two host-clock figures between two device synchronisations: the
whole interval with nothing waited for inside it, and what comes behind iterate() alone (the overhead).

--loop plant: the closed loop of planner and plant under a plant whose parameters are 5 % off and whose state is disturbed
at every step, `--rounds` control intervals per loop, in three forms that ALTERNATE in one process:
    receding_plant   BatchSolver.receding_plant: one call, the loop on the device (k_plant)
    composed         the same loop driven from Python out of the public device entries: policy_rollout(device=True, params=...)
                     with one start per trajectory and whole roll-outs, a torch add for the disturbance, shift(cuda tensors)
    receding         BatchSolver.receding: the model loop, which has no plant (nothing is measured, no gain is used)
Per form and repeat two host-clock figures between two device synchronisations, both divided by the rounds: the whole loop
with `--iterations` solver iterations per round, and the loop with 0 iterations per round behind one iterate() — what a
round costs behind its iterations (the overhead).  receding_plant's figures include its one upload of the tables and its one
download of the logs, receding's its one download.  k_plant's own time is HIP events.

--loop windows: tracking MPC, the model loop of a problem whose per-time-step parameter has a window per trajectory (almix
FULL_DDP 1, `vref`, rows; --config is not read), `--rounds` control intervals per loop, in three forms that ALTERNATE in one
process:
    resident         BatchSolver.receding(windows=...): one call, every window moved on the device by k_shift_windows from a
                     future sent once
    hand, device     the loop from Python with the tails on the GPU: iterate; head(device=True); shift_param_batch(device=True)
                     with the round's columns of a torch tensor; shift
    hand, host       the same with host tails: iterate; head; shift_param_batch(numpy columns); shift
Figures as for --loop plant: per round the whole loop, and the loop with 0 iterations per round behind one iterate() (the
overhead behind iterate).  The resident form's figures include its one upload of the future and its one download of the log.
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


def run_external(ilqg, synth, config, repeats, steps, warmup, iterations):
    import torch
    if config == "headline":
        problem, fd, B, N, params = "carparking", 0, 65536, 500, ilqg.CAR_PARAMS
        x0, u0 = synth.car_batch(B, N)
    else:
        problem, fd, B, N, params = "synth16x8", 1, 16384, 1000, synth.SYNTH16_PARAMS
        x0, u0 = synth.synth16_batch(B, N)
    s = ilqg.BatchSolver(problem, fd, batch=B, n_hor=N, params=params, opts=dict(max_iter=1 << 20))
    nx, nu = s.problem.nx, s.problem.nu
    print("== %s: %s FULL_DDP=%d, %d trajectories, N = %d, %d step(s) applied per interval, %d iteration(s) per interval, %d stream group(s), %s mapping" % (
        config, problem, fd, B, N, steps, iterations, s.groups(), "wave" if s.problem.wave_mapping else "lane"))
    rng = np.random.default_rng(1)
    noise = 1e-3 * rng.standard_normal((B, nx))
    noise_t = torch.from_numpy(noise).cuda()
    walk = [np.array(x0, dtype=np.float64)]
    applied = {}

    def host_u():  # the parent's form without the states: the plant cannot see the plan's x[steps]
        applied["u"] = s.u()[:, :steps]
        walk[0] = walk[0] + noise
        s.shift(steps, walk[0])

    def host_xu():  # the parent's form with the plant of the device form
        applied["u"] = s.u()[:, :steps]
        s.shift(steps, s.x()[:, steps] + noise)

    def device():
        h = s.head(steps + 1, device=True)
        applied["u"] = h["u"][:, :steps]
        s.shift(steps, h["x"][:, steps] + noise_t)

    forms = (("host: u(), shift(x_meas on the host)", host_u), ("host: u(), x(), shift(x_meas on the host)", host_xu),
             ("device: head(device=True), shift(x_meas on the GPU)", device))

    def sync():
        torch.cuda.synchronize()
        s.sync()

    s.init(x0, u0)
    s.iterate(warmup)
    for _, f in forms:  # once untimed: staging buffers, torch's allocator
        s.iterate(iterations)
        f()
    sync()
    s.timing(True)
    whole, over = {n: [] for n, _ in forms}, {n: [] for n, _ in forms}
    layout, seen = {n: [0, 0.0] for n, _ in forms}, [0, 0.0]  # "layout kernels" per form: read between the timed regions
    for r in range(repeats):
        for name, f in forms:
            sync()
            t0 = time.perf_counter()
            s.iterate(iterations)
            f()
            sync()
            whole[name].append(1e3 * (time.perf_counter() - t0))
            s.iterate(iterations)
            sync()
            t0 = time.perf_counter()
            f()
            sync()
            over[name].append(1e3 * (time.perf_counter() - t0))
            n, ms = s.kernel_times()["layout kernels"]
            layout[name][0] += n - seen[0]
            layout[name][1] += ms - seen[1]
            seen = [n, ms]
    kt = s.kernel_times()
    s.timing(False)
    for name, _ in forms:
        print("%-52s interval  %s" % (name, spread(whole[name])))
        print("%-52s overhead  %s" % ("", spread(over[name])))
    dev = forms[2][0]
    for name, _ in forms[:2]:
        print("ratio of medians, %s / device: interval %.2f, overhead %.1f" % (
            name.split(",")[0] + ("+x()" if "x()" in name else ""), np.median(whole[name]) / np.median(whole[dev]), np.median(over[name]) / np.median(over[dev])))
    n, ms = kt["k_head"]
    print("k_head: %d launches, %.4f ms per launch (%d bytes per trajectory out)" % (n, ms / max(n, 1), ((steps + 1) * nx + (steps + 1) * nu + 1) * 8))
    for name, _ in forms:  # device form: the scatter of x0_new (k_nom_io, k_to_dev); host forms: the transposes of u(), x(), x0_new
        n, ms = layout[name]
        print("layout kernels, %-52s %d launches, %.4f ms per control interval (sum over the groups)" % (name + ":", n, ms / (2 * repeats)))
    n, ms = kt["k_shift"]
    print("k_shift: %d launches, %.3f ms per launch; k_rollout[init]: %.3f ms per launch (every form)" % (
        n, ms / max(n, 1), kt["k_rollout[init]"][1] / max(kt["k_rollout[init]"][0], 1)))
    print("through the host per interval: u() %.2f GB, x() %.2f GB; device form: nothing" % (B * N * nu * 8 / 1e9, B * (N + 1) * nx * 8 / 1e9))
    s.close()


def run_plant(ilqg, synth, config, repeats, steps, warmup, iterations, rounds):
    import torch
    if config == "headline":
        problem, fd, B, N, params, names = "carparking", 0, 65536, 500, ilqg.CAR_PARAMS, ("limA", "d", "cf", "cx")
        x0, u0 = synth.car_batch(B, N)
    else:
        problem, fd, B, N, params, names = "synth16x8", 1, 16384, 1000, synth.SYNTH16_PARAMS, ("qf", "c", "lim")
        x0, u0 = synth.synth16_batch(B, N)
    s = ilqg.BatchSolver(problem, fd, batch=B, n_hor=N, params=params, opts=dict(max_iter=1 << 20))
    nx, nu = s.problem.nx, s.problem.nu
    print("== %s: %s FULL_DDP=%d, %d trajectories, N = %d, %d round(s) per loop, %d step(s) applied and %d iteration(s) per round, %d stream group(s), %s mapping" % (
        config, problem, fd, B, N, rounds, steps, iterations, s.groups(), "wave" if s.problem.wave_mapping else "lane"))
    rng = np.random.default_rng(1)
    rows = {n: np.asarray(params[n], dtype=np.float64).reshape(-1) * (1.0 + 0.05 * rng.standard_normal((B, np.size(params[n])))) for n in names}
    W = sum(t.shape[1] for t in rows.values())
    w = 1e-3 * rng.standard_normal((B, rounds * steps, nx))
    rows_t = {n: torch.from_numpy(t[:, None].copy()).cuda() for n, t in rows.items()}
    w_t = torch.from_numpy(np.ascontiguousarray(w.transpose(1, 0, 2))).cuda()  # [rounds * steps][B][nx]
    state = {}

    def start():  # every loop begins with plants at their plans' x_0
        state["xp"] = s.head(1)["x"][:, 0].copy()

    def plant(k):
        s.receding_plant(rounds, steps, k, True, state["xp"], rows, w)

    def composed(k):
        xp = torch.from_numpy(state["xp"]).cuda()
        for r in range(rounds):
            s.iterate(k)
            o = s.policy_rollout(xp[:, None].contiguous(), alpha=0.0, feedback=True, trajectories=True, device=True, params=rows_t)
            xp = o["x"][:, 0, steps] + w_t[r * steps + steps - 1]  # (steps > 1: the disturbances inside a roll-out are left out)
            state["logs"] = (o["x"][:, 0, :steps], o["u"][:, 0, :steps])
            s.shift(steps, xp.contiguous())

    def model(k):
        s.receding(rounds, steps, k)

    forms = (("receding_plant (k_plant, one call)", plant), ("composed from policy_rollout / torch / shift", composed), ("receding (no plant)", model))

    def sync():
        torch.cuda.synchronize()
        s.sync()

    s.init(x0, u0)
    s.iterate(warmup)
    for _, f in forms:  # once untimed: the logs' and staging buffers, torch's allocator
        start()
        f(iterations)
    sync()
    s.timing(True)
    whole, over = {n: [] for n, _ in forms}, {n: [] for n, _ in forms}
    for r in range(repeats):
        for name, f in forms:
            start()
            sync()
            t0 = time.perf_counter()
            f(iterations)
            sync()
            whole[name].append(1e3 * (time.perf_counter() - t0) / rounds)
            s.iterate(iterations)  # the first round of the overhead loop finds the batch as a round behind its iterations does
            start()
            sync()
            t0 = time.perf_counter()
            f(0)
            sync()
            over[name].append(1e3 * (time.perf_counter() - t0) / rounds)
    kt = s.kernel_times()
    s.timing(False)
    for name, _ in forms:
        print("%-48s per round  %s" % (name, spread(whole[name])))
        print("%-48s overhead   %s" % ("", spread(over[name])))
    new, comp, base = (np.median(over[n]) for n, _ in forms)
    n, ms = kt["k_plant"]
    per_launch = ms / max(n, 1)
    print("k_plant: %d launches, %.4f ms per launch (%d per round: one per stream group); the table is %d doubles per trajectory" % (n, per_launch, s.groups(), W))
    print("overhead per round, medians: receding_plant %.3f ms, composed %.3f ms (%.1f x), receding %.3f ms; receding_plant - receding = %.3f ms against "
          "%.3f ms of k_plant launches per round" % (new, comp, comp / new, base, new - base, per_launch * s.groups()))
    n, ms = kt["k_policy_params"]
    print("k_policy_params (composed form): %d launches, %.3f ms per launch; k_shift %.3f ms, k_rollout[init] %.3f ms per launch (every form)" % (
        n, ms / max(n, 1), kt["k_shift"][1] / max(kt["k_shift"][0], 1), kt["k_rollout[init]"][1] / max(kt["k_rollout[init]"][0], 1)))
    s.close()


def run_windows(ilqg, repeats, steps, warmup, iterations, rounds, batch):
    import torch
    from oracle.harness import almix_case
    name, B = "vref", batch
    params, opts, x0, u0 = almix_case(batch=B)
    N = u0.shape[1]
    s = ilqg.BatchSolver("almix", 1, batch=B, n_hor=N, params=params, opts=dict(opts, max_iter=1 << 20))
    print("== almix FULL_DDP=1, %d trajectories, N = %d, a window of `vref` per trajectory, %d round(s) per loop, %d step(s) applied and %d iteration(s) "
          "per round, %d stream group(s)" % (B, N, rounds, steps, iterations, s.groups()))
    rng = np.random.default_rng(59)
    per = rounds * steps
    T = (0.8 + 0.4 * np.sin(0.2 * np.arange(N + 1 + per)))[None, :] * (1.0 + 0.05 * rng.standard_normal((B, N + 1 + per)))
    rows, future = np.ascontiguousarray(T[:, :N + 1]), np.ascontiguousarray(T[:, N + 1:])
    tails = [np.ascontiguousarray(future[:, r * steps:(r + 1) * steps]) for r in range(rounds)]
    tails_t = [torch.from_numpy(t).cuda() for t in tails]
    kept = {}

    def resident(k):
        kept["log"] = s.receding(rounds, steps, k, windows={name: future})

    def hand_device(k):
        for r in range(rounds):
            s.iterate(k)
            kept["head"] = s.head(steps, device=True)
            s.shift_param_batch(name, steps, tails_t[r], device=True)
            s.shift(steps)

    def hand_host(k):
        for r in range(rounds):
            s.iterate(k)
            kept["head"] = s.head(steps)
            s.shift_param_batch(name, steps, tails[r])
            s.shift(steps)

    forms = (("resident: receding(windows=...), one call", resident), ("hand loop, tails on the GPU", hand_device), ("hand loop, tails on the host", hand_host))

    def sync():
        torch.cuda.synchronize()
        s.sync()

    s.set_param_steps_batch(name, rows)
    s.init(x0, u0)
    s.iterate(warmup)
    for _, f in forms:  # once untimed: the logs', futures' and staging buffers, torch's allocator
        f(iterations)
    sync()
    s.timing(True)
    whole, over = {n: [] for n, _ in forms}, {n: [] for n, _ in forms}
    for r in range(repeats):
        for label, f in forms:
            sync()
            t0 = time.perf_counter()
            f(iterations)
            sync()
            whole[label].append(1e3 * (time.perf_counter() - t0) / rounds)
            s.iterate(iterations)  # the first round of the overhead loop finds the batch as a round behind its iterations does
            sync()
            t0 = time.perf_counter()
            f(0)
            sync()
            over[label].append(1e3 * (time.perf_counter() - t0) / rounds)
    kt = s.kernel_times()
    s.timing(False)
    for label, _ in forms:
        print("%-48s per round  %s" % (label, spread(whole[label])))
        print("%-48s overhead   %s" % ("", spread(over[label])))
    res, dev, host = (np.median(over[n]) for n, _ in forms)
    print("overhead per round behind iterate, medians: resident %.3f ms, hand loop with device tails %.3f ms (%.2f x), with host tails %.3f ms (%.2f x)" % (
        res, dev, dev / res, host, host / res))
    for k in ("k_shift_windows", "k_shift_param_rows", "k_shift", "k_log_steps", "k_head", "k_rollout[init]"):
        n, ms = kt[k]
        print("%s: %d launches, %.4f ms per launch" % (k, n, ms / max(n, 1)))
    print("a window is %d doubles per trajectory; per round and trajectory %d of them come from the future" % (N + 1, steps))
    s.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="both", choices=("headline", "config5", "both"))
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--steps", type=int, default=None, help="steps per shift (default 10; 1 with --loop external / plant)")
    ap.add_argument("--loop", default="replan", choices=("replan", "external", "plant", "windows"),
                    help="external: the control interval of a caller with its own plant; plant: the closed loop of planner and plant on the device; "
                         "windows: the model loop with a moving window per trajectory (almix)")
    ap.add_argument("--batch", type=int, default=65536, help="--loop windows: trajectories")
    ap.add_argument("--iterations", type=int, default=2, help="--loop external / plant: solver iterations per control interval")
    ap.add_argument("--rounds", type=int, default=None, help="--loop plant / windows: control intervals per timed loop (default 5; 10 with --loop windows)")
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--between", type=int, default=2, help="solver iterations between two re-plans")
    a = ap.parse_args()
    import __graft_entry__ as g
    g.load_package()
    from ddp_generator_amd import ilqg, synth
    if a.loop == "windows":
        run_windows(ilqg, a.repeats, a.steps or 1, a.warmup, a.iterations, a.rounds or 10, a.batch)
        return
    for config in (("headline", "config5") if a.config == "both" else (a.config,)):
        if a.loop == "external":
            run_external(ilqg, synth, config, a.repeats, a.steps or 1, a.warmup, a.iterations)
        elif a.loop == "plant":
            run_plant(ilqg, synth, config, a.repeats, a.steps or 1, a.warmup, a.iterations, a.rounds or 5)
        else:
            run(ilqg, synth, config, a.repeats, a.steps or 10, a.warmup, a.between)


if __name__ == "__main__":
    main()
