#!/usr/bin/env python3
"""Roll-outs of the policy from perturbed starts (BatchSolver.policy_rollout, k_policy) against the line search's roll-outs.

    python tools/policy_profile.py [--config headline|config5|both] [--repeats 10] [--warmup 3] [--rs 1,8,64] [--scalar-search] [--params] [--noise] [--drawn]

One process per invocation, one stream group (a launch's HIP-event time is then that launch alone).  The yardstick is the
line search of the SAME run with ls_keep = 0, ls_split = 0: k_rollout[search] rolls out (active trajectories) x n_alpha
chains with the same arithmetic per step, one lane per roll-out, and keeps the costs only.  After `--warmup` iterations
the legs ALTERNATE, `--repeats` times: one solver iteration (its search launch is the yardstick), costs-only roll-outs of
the policy at every R of --rs, whole roll-outs at R = 8 (device form: the outputs stay on the GPU), and R = 8 costs-only
through the host form against the device form (host clock between two device synchronisations).  Kernel times are HIP
events (ilqg_batch_get_timing), read before and after every leg.  Not part of bench.py.

--params adds the roll-outs under parameters per roll-out (policy_rollout(params=...), k_policy<true>, timing slot
"k_policy_params") to the same alternation: costs only at every R of --rs with ALL fixed-size parameters named and with a
SINGLE parameter named, each roll-out with a row of its own ([B, R, W], nominal * (1 + 0.05 N(0, 1))), and at R = 8 one
[R, W] table shared by every trajectory against the per-trajectory table.  Each is reported as a ratio to the plain k_policy
launch of the same R in the same run.

--noise adds the roll-outs under a disturbance table (policy_rollout(disturbance=...), the same k_policy with a table argument)
to the same alternation: R = 8, costs only, device form, with a table per roll-out ([B, R, N, nx], 0.01 N(0, 1) drawn on the
GPU) and with one [R, N, nx] table shared by every trajectory, each as a ratio to the plain k_policy launch at R = 8 of the
same run (the leg "device R=8").  That plain launch is also what a build of the parent commit is compared with — the same
tool run there, alternating with this one: a null table is meant to cost nothing measurable.

--drawn (implies --noise) adds the roll-outs whose noise is drawn on the device (policy_rollout(noise=(seed, sigma)),
k_policy_drawn, a timing slot of its own) to the same alternation, costs only, device form: R = 8 with noise per trajectory and
with shared noise, as ratios to the plain launch, to the launch under a table per roll-out and to the launch under the shared
table of the same run; and R = 64, drawn only, with the size of the table it does without.  noise_table (k_noise_fill) at R = 8
is timed too.  No bar is set on these ratios: they are findings.
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def spread(v, unit="ms"):
    v = np.asarray(v, dtype=np.float64)
    return "median %10.4f %s  min %10.4f  max %10.4f  (n = %d)" % (np.median(v), unit, v.min(), v.max(), len(v))


def run(ilqg, synth, config, repeats, warmup, rs, scalar_search, with_params=False, with_noise=False, with_drawn=False):
    import torch
    if scalar_search:  # (read once, when the context is made)
        os.environ["ILQG_NO_ROLLOUT_PARTS"] = "1"
    else:
        os.environ.pop("ILQG_NO_ROLLOUT_PARTS", None)
    if config == "headline":
        problem, fd, B, N, params = "carparking", 0, 65536, 500, ilqg.CAR_PARAMS
        x0, u0 = synth.car_batch(B, N)
    else:
        problem, fd, B, N, params = "synth16x8", 1, 16384, 1000, synth.SYNTH16_PARAMS
        x0, u0 = synth.synth16_batch(B, N)
    s = ilqg.BatchSolver(problem, fd, batch=B, n_hor=N, params=params, opts=dict(max_iter=1 << 20, ls_keep=0, ls_split=0), groups=1)
    nx, nu = s.problem.nx, s.problem.nu
    print("== %s: %s FULL_DDP=%d, %d trajectories, N = %d, %d stream group(s), %s mapping, ls_keep = 0, ls_split = 0%s" % (
        config, problem, fd, B, N, s.groups(), "wave" if s.problem.wave_mapping else "lane",
        ", ILQG_NO_ROLLOUT_PARTS=1 (the search on k_rollout, one lane per roll-out, where the build has the step in parts)" if scalar_search else ""), flush=True)
    s.init(x0, u0)
    s.iterate(warmup)
    s.sync()
    rng = np.random.default_rng(3)
    plan_x0 = s.head(1)["x"][:, 0]
    rmax = max(rs + [8] + ([64] if with_drawn else []))
    starts = torch.from_numpy(plan_x0[:, None, :] + 0.1 * rng.standard_normal((B, rmax, nx))).cuda()
    dev_starts = {R: starts[:, :R].contiguous() for R in set(rs + [8] + ([64] if with_drawn else []))}
    host8 = dev_starts[8].cpu().numpy()

    def sync():
        torch.cuda.synchronize()
        s.sync()

    def kernel(name):
        n, ms = s.kernel_times().get(name, (0, 0.0))
        return n, ms

    legs = [("search", None)] + [("costs R=%d" % R, R) for R in rs] + [("whole R=8", 8), ("host R=8", 8), ("device R=8", 8)]
    tables = {}
    if with_params:
        fixed = [(n, size) for n, size in s.problem.params if size > 0]
        single = fixed[0][0]
        gen = torch.Generator(device="cuda").manual_seed(5)

        def table(names, shape):
            return {n: torch.tensor(np.asarray(params[n], dtype=np.float64).reshape(-1), device="cuda") *
                    (1.0 + 0.05 * torch.randn(shape + (size,), dtype=torch.float64, device="cuda", generator=gen)) for n, size in fixed if n in names}
        for R in rs:
            tables["all R=%d" % R] = table([n for n, _ in fixed], (B, R))
            tables["one R=%d" % R] = table([single], (B, R))
            legs += [("all R=%d" % R, R), ("one R=%d" % R, R)]
        if 8 not in rs:
            tables["all R=8"] = table([n for n, _ in fixed], (B, 8))
            legs.append(("all R=8", 8))
        tables["shared R=8"] = table([n for n, _ in fixed], (8,))
        legs.append(("shared R=8", 8))
        print("   --params: %d fixed-size parameters, %d doubles per row when all are named (%s); the single one is %s" % (
            len(fixed), sum(size for _, size in fixed), ", ".join(n for n, _ in fixed), single), flush=True)

    noise = {}
    if with_noise:
        gen_w = torch.Generator(device="cuda").manual_seed(7)
        # (scaled in place: a second copy of the table per roll-out is 8 or 17 GB more of the device's memory)
        noise["noise full R=8"] = torch.randn((B, 8, N, nx), dtype=torch.float64, device="cuda", generator=gen_w).mul_(0.01)
        noise["noise shared R=8"] = torch.randn((8, N, nx), dtype=torch.float64, device="cuda", generator=gen_w).mul_(0.01)
        legs += [(name, 8) for name in noise]
        print("   --noise: a table per roll-out of %.2f GB, a shared one of %.1f KB" % (B * 8 * N * nx * 8 / 1e9, 8 * N * nx * 8 / 1e3), flush=True)

    drawn = {}
    if with_drawn:
        sigma = np.full(nx, 0.01)
        drawn = {"drawn R=8": (8, False), "drawn shared R=8": (8, True), "drawn R=64": (64, False), "fill R=8": (8, False)}
        legs += [(name, R) for name, (R, _) in drawn.items()]
        print("   --drawn: seed 20261021, sigma 0.01; at R = 64 a table per roll-out would be %.1f GB" % (B * 64 * N * nx * 8 / 1e9), flush=True)

    def slot(name):
        return ("k_rollout[search]" if name == "search" else "k_policy_params" if name in tables else "k_noise_fill" if name.startswith("fill")
                else "k_policy_drawn" if name in drawn else "k_policy")

    def leg(name, R):
        if name.startswith("fill"):
            s.noise_table(R, 20261021, sigma, device=True)
        elif name in drawn:
            s.policy_rollout(dev_starts[R], device=True, noise=(20261021, sigma), noise_shared=drawn[name][1])
        elif name in noise:
            s.policy_rollout(dev_starts[R], device=True, disturbance=noise[name])
        elif name in tables:
            s.policy_rollout(dev_starts[R], device=True, params=tables[name])
        elif name == "search":
            s.iterate(1)
        elif name.startswith("costs") or name.startswith("device"):
            s.policy_rollout(dev_starts[R], device=True)
        elif name.startswith("whole"):
            s.policy_rollout(dev_starts[R], trajectories=True, device=True)
        else:
            s.policy_rollout(host8)

    for name, R in legs:  # once untimed: staging buffers, torch's allocator, scratch memory
        t0 = time.perf_counter()
        leg(name, R)
        sync()
        print("   (untimed first call, %-12s %9.1f ms of wall clock)" % (name + ":", 1e3 * (time.perf_counter() - t0)), flush=True)
    s.timing(True)
    kern = {name: [] for name, _ in legs}   # ms per launch of the leg's kernel
    wall = {name: [] for name, _ in legs}   # host clock between two synchronisations
    per = {name: [] for name, _ in legs}    # ns per roll-out
    actives = []
    n_alpha = 8  # standard_parameters (iLQG.c:74): no option of this run changes the list of step sizes
    for r in range(repeats):
        for name, R in legs:
            which = slot(name)
            active = s.active() if name == "search" else B
            sync()
            n0, ms0 = kernel(which)
            t0 = time.perf_counter()
            leg(name, R)
            sync()
            wall[name].append(1e3 * (time.perf_counter() - t0))
            n1, ms1 = kernel(which)
            kern[name].append((ms1 - ms0) / max(n1 - n0, 1))
            if name == "search":
                rollouts = active * n_alpha
                actives.append(active)
            else:
                rollouts = B * R
            per[name].append(1e6 * (ms1 - ms0) / max(rollouts, 1))
    s.timing(False)
    print("the searches rolled out %d .. %d active trajectories x %d step sizes" % (min(actives), max(actives), n_alpha))
    for name, R in legs:
        which = slot(name)
        print("%-12s %-18s per launch   %s" % (name, which, spread(kern[name])))
        print("%-12s %-18s per roll-out %s" % ("", "", spread(per[name], "ns")))
    base = np.median(per["search"])
    lo, hi = np.min(per["search"]), np.max(per["search"])
    for name, R in legs[1:len(rs) + 2]:
        m = np.median(per[name])
        print("ratio per roll-out, k_policy %-10s / k_rollout[search]: %.3f  (medians; the search's own repeats span %.3f .. %.3f of its median, k_policy's %.3f .. %.3f of its)" % (
            name, m / base, lo / base, hi / base, np.min(per[name]) / m, np.max(per[name]) / m))
    for name, R in legs:
        if name not in tables:
            continue
        plain = "costs R=%d" % R if R in rs else "device R=8"
        m, p0 = np.median(kern[name]), np.median(kern[plain])
        print("ratio per launch, k_policy_params %-11s / k_policy %-11s: %.3f  (medians; its repeats span %.3f .. %.3f of its median, the plain launch's %.3f .. %.3f of its)" % (
            name, plain, m / p0, np.min(kern[name]) / m, np.max(kern[name]) / m, np.min(kern[plain]) / p0, np.max(kern[plain]) / p0))
    for name in noise:
        m, p0 = np.median(kern[name]), np.median(kern["device R=8"])
        print("ratio per launch, k_policy %-16s / k_policy device R=8 (no table): %.3f  (medians; its repeats span %.3f .. %.3f of its median, the plain launch's %.3f .. %.3f of its)" % (
            name, m / p0, np.min(kern[name]) / m, np.max(kern[name]) / m, np.min(kern["device R=8"]) / p0, np.max(kern["device R=8"]) / p0))
    if with_drawn:
        def ratio(a, b, what):
            m, p0 = np.median(kern[a]), np.median(kern[b])
            print("ratio per launch, %-44s %.3f  (medians; its repeats span %.3f .. %.3f of its median, the other's %.3f .. %.3f of its)" % (
                what + ":", m / p0, np.min(kern[a]) / m, np.max(kern[a]) / m, np.min(kern[b]) / p0, np.max(kern[b]) / p0))
        ratio("drawn R=8", "device R=8", "drawn / plain, R = 8")
        ratio("drawn R=8", "noise full R=8", "drawn / table per roll-out, R = 8")
        ratio("drawn shared R=8", "noise shared R=8", "drawn shared / shared table, R = 8")
        if 64 in rs:
            ratio("drawn R=64", "costs R=64", "drawn / plain, R = 64")
        print("drawn R=64: %.4f ms per launch (median), %.2f ns per roll-out; the table it does without: %.1f GB" % (
            np.median(kern["drawn R=64"]), np.median(per["drawn R=64"]), B * 64 * N * nx * 8 / 1e9))
        print("noise_table R=8 (k_noise_fill, %.2f GB written): %.4f ms per launch (median)" % (B * 8 * N * nx * 8 / 1e9, np.median(kern["fill R=8"])))
    if with_params:
        print("ratio per launch, shared [R, W] table / per-trajectory [B, R, W] table at R = 8, all parameters named: %.3f" % (
            np.median(kern["shared R=8"]) / np.median(kern["all R=8"])))
    print("host form R=8, host clock:    " + spread(wall["host R=8"]))
    print("device form R=8, host clock:  " + spread(wall["device R=8"]))
    print("ratio of medians host / device form: %.2f  (host form: %.1f MB of starts up, %.1f MB of results down per call)" % (
        np.median(wall["host R=8"]) / np.median(wall["device R=8"]), B * 8 * nx * 8 / 1e6, B * 8 * (8 + 4 + nx * 8) / 1e6))
    print("whole roll-outs at R=8 write %.2f GB per call (x and u, scattered 8-byte stores per lane)" % (B * 8 * ((N + 1) * nx + N * nu) * 8 / 1e9))
    s.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="both", choices=("headline", "config5", "both"))
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rs", default="1,8,64")
    ap.add_argument("--scalar-search", action="store_true", help="wave-mapped builds whose line search rolls out in parts (k_rollout_parts, "
                    "several wavefronts per 64 trajectories): the search on k_rollout instead, one lane per roll-out like k_policy")
    ap.add_argument("--params", action="store_true", help="also the roll-outs under parameters per roll-out (k_policy_params): all fixed-size "
                    "parameters named, a single one named, and a shared against a per-trajectory table at R = 8")
    ap.add_argument("--noise", action="store_true", help="also the roll-outs under a disturbance table at R = 8, costs only: a table per roll-out "
                    "and one shared by every trajectory, as ratios to the plain launch of the same run")
    ap.add_argument("--drawn", action="store_true", help="also the roll-outs whose noise is drawn on the device (k_policy_drawn) at R = 8 and "
                    "R = 64, costs only, as ratios to the plain launch and to the launches under a table (implies --noise)")
    a = ap.parse_args()
    import __graft_entry__ as g
    g.load_package()
    from ddp_generator_amd import ilqg, synth
    for config in (("headline", "config5") if a.config == "both" else (a.config,)):
        run(ilqg, synth, config, a.repeats, a.warmup, [int(r) for r in a.rs.split(",")], a.scalar_search, a.params, a.noise or a.drawn, a.drawn)


if __name__ == "__main__":
    main()
