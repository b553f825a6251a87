#!/usr/bin/env python3
"""Batch of independent QPs (BASELINE configs[3]: 1024 x (n=512, m=256)) on one GPU / one rank.

    python tools/bench_batch.py [--batch 128] [--nx 512] [--m 256] [--streams 16] [--mixed-patterns [SEED]]
                                [--refine-steps N] [--trace] [--shared [SEED]]

Under torch.distributed.run each rank takes problems rank, rank+N, ... (no communication) and rank 0
reports the aggregate.  Prints one JSON line: QPs/s and IPM iterations/s.

--mixed-patterns: the same problems, each with a bound / row pattern of its own drawn from SEED (some variables free,
lower-only or upper-only; some rows equalities or one-sided), through the engine's per-problem patterns -- timed in
the same call, alternately with the problems under their one shared pattern; the line then holds both and the ratio
of problem-iterations per second (the sum of per-problem iterations over wall time).

--refine-steps N / --trace: passed through to BatchedMPCSolver (N steps of iterative refinement in every solve; the
per-iteration trace, recorded on the device and read back inside the timed region); the line names both.

--shared: the parametric batch -- ONE model (the first problem's H and A) with q, variable bounds and row bounds of
their own per problem, drawn from SEED -- solved alternately in the stacked form (every problem holds clones of H and A)
and with shared_matrices=True (one H, one A: madqp_batch_share_matrices).  The line's own figures are the stacked form's;
"shared_matrices" holds, for both forms, QP/s, the set-up time (constructor + initialize), the device bytes the solver
holds beyond the caller's problem data (free device memory before and after set-up, allocator caches emptied: the
library's own arrays included), whether the two forms agree bitwise, and the roofline on the shared algorithmic bytes.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402


def batch_roofline(nx, m, iters, seconds, max_ncorr=0, shared_batch=0):
    """Where a batch of small QPs stands against the chip's two bounds (whole-run averages).
    MFMA flops per problem-iteration: assembly m nx^2 + Cholesky nx^3/3.
    Algorithmic HBM bytes per problem-iteration: every matrix pass the iteration needs at 8 B per entry, a pass over a
    triangle counted as half a matrix -- per solve_system (two at max_ncorr = 0): A' u, A dx, A' v_y (m nx each; the
    residual check reuses the solve's A dx), H v from the lower triangle (nx^2/2), two sweeps over L (nx^2/2 each); per
    iteration besides: jtprod A' y (m nx), the model evaluation H x + A x (nx^2/2 + m nx); assembly: H lower (nx^2/2) in, the scaled operand
    sqrt(Theta) A written and read (2 m nx), K lower out (nx^2/2); Cholesky: K in, L out (nx^2/2 each).
    shared_batch = B > 0: the batch shares ONE H and ONE A (shared_matrices=True) -- every pass over A or H above is counted
    once per batch-iteration, i.e. 1/B of it per problem, and the assembly's addend is the scaled lower triangle written into
    K first (nx^2/2 out, nx^2/2 in, in place of H lower in)."""
    flops = m * nx * nx + nx ** 3 / 3.0
    solves = 2 + max_ncorr
    a_passes, h_passes = (solves * 3 + 2) * m * nx, (solves + 2) * (nx * nx // 2)  # (the last H pass: the assembly's addend)
    rest = solves * nx * nx + (2 * m * nx + nx * nx // 2) + nx * nx
    if shared_batch:
        doubles = rest + (m * nx + nx * nx // 2) / shared_batch + 2 * (nx * nx // 2)
    else:
        doubles = a_passes + h_passes + rest
    it_per_s = iters / seconds
    tf, gbs = it_per_s * flops * 1e-12, it_per_s * 8.0 * doubles * 1e-9
    return {"flops_per_problem_iteration": flops, "algorithmic_bytes_per_problem_iteration": 8.0 * doubles,
            "achieved_TFLOPs": tf, "frac_of_fp64_mfma_peak": tf / bench.PEAK_F64_MFMA_TFLOPS,
            "achieved_GBps_algorithmic": gbs, "frac_of_hbm_peak": gbs / bench.PEAK_HBM_GBS}


def mixed_patterns(qps, seed):
    """Copies of ``qps`` (DeviceQP, same data) with a pattern of their own each, drawn from ``seed``: variables 10 % free,
    15 % lower-only, 15 % upper-only, the rest boxed; rows 10 % equalities (at 0.1), 15 % lower-only, 15 % upper-only."""
    import copy

    import numpy as np
    import torch

    rng = np.random.default_rng(seed)
    out = []
    for dq in qps:
        v = torch.as_tensor(rng.random(dq.nvar), device=dq.lvar.device)
        r = torch.as_tensor(rng.random(dq.ncon), device=dq.lcon.device)
        c = copy.copy(dq)
        inf = float("inf")
        c.lvar = torch.where((v < 0.10) | ((v >= 0.25) & (v < 0.40)), -inf, dq.lvar)
        c.uvar = torch.where(v < 0.25, inf, dq.uvar)
        c.lcon = torch.where(r < 0.10, 0.1, torch.where((r >= 0.25) & (r < 0.40), -inf, dq.lcon))
        c.ucon = torch.where(r < 0.10, 0.1, torch.where((r >= 0.10) & (r < 0.25), inf, dq.ucon))
        out.append(c)
    return out


def one_model(M, qps, seed):
    """``qps`` (DeviceQP) turned into a parametric batch: every problem gets problem 0's H and A, keeps its own q and gets
    bounds of its own (each finite bound moved outwards by up to 10 % of a unit, drawn from ``seed``).  Returns
    (stacked, shared): the same problems holding clones of H and A, and holding the ONE H and A."""
    import copy

    import numpy as np
    import torch

    rng = np.random.default_rng(seed)
    H, A = qps[0].H, qps[0].A
    stacked, shared = [], []
    for dq in qps:
        c = copy.copy(dq)
        r = lambda t: torch.as_tensor(0.1 * rng.random(t.numel()), device=t.device)
        c.lvar, c.uvar, c.lcon, c.ucon = dq.lvar - r(dq.lvar), dq.uvar + r(dq.uvar), dq.lcon - r(dq.lcon), dq.ucon + r(dq.ucon)
        c.H, c.A = H, A
        shared.append(c)
        k = copy.copy(c)
        k.H, k.A = None if H is None else H.clone(), A.clone()
        stacked.append(k)
    return stacked, shared


def held_bytes():
    """Device memory in use (all allocators of this process, and of others on the device), allocator caches emptied."""
    import torch

    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    free, total = torch.cuda.mem_get_info()
    return total - free


def run_batched(M, be, batch, nx, m, seed, repeats=3, check_every=2, profile=False):
    """The lock-step batched engine on `batch` synthetic QPs of this rank: (median seconds, results, all times)."""
    import torch

    opts = dict(max_iter=300, step_rule=M.AdaptiveStep(0.995), regularization=M.FixedRegularization(1e-8, -1e-8),
                mu_min=1e-12)
    qps = [M.DeviceQP.synthetic(be, seed + i, nx, m) for i in range(batch)]
    warm = M.BatchedMPCSolver(qps, be, **opts)
    warm.solve(check_every=check_every)
    warm.close()
    times, res = [], None
    for _ in range(max(1, repeats)):
        solver = M.BatchedMPCSolver(qps, be, **opts)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        res = solver.solve(check_every=check_every)
        torch.cuda.synchronize()
        times.append(time.perf_counter() - t0)
        solver.close()
    return sorted(times)[len(times) // 2], res, times


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--batch", type=int, default=128)
    p.add_argument("--nx", type=int, default=512)
    p.add_argument("--m", type=int, default=256)
    p.add_argument("--streams", type=int, default=16)
    p.add_argument("--seed", type=int, default=20250614 + 3)
    p.add_argument("--driver", choices=("native", "python"), default="native")
    p.add_argument("--engine", choices=("batched", "streams"), default="batched",
                   help="batched: lock-step engine of csrc/batch.hip; streams: one MPCSolver per problem, "
                        "several HIP streams in flight (madqp_jl_amd/batch.py)")
    p.add_argument("--check-every", type=int, default=2)
    p.add_argument("--repeats", type=int, default=3, help="timed solves (fresh solver each); the median is reported")
    p.add_argument("--profile", action="store_true", help="print ms / launches per kernel class (perturbs timing)")
    p.add_argument("--mixed-patterns", type=int, nargs="?", const=1, default=None, metavar="SEED",
                   help="also solve the problems with a pattern of their own each (per_problem_patterns=True), "
                        "alternately with the shared pattern; reports both (batched engine only)")
    p.add_argument("--refine-steps", type=int, default=None, metavar="N",
                   help="refine_steps of the batched engine (default: the solver's own default, 0)")
    p.add_argument("--trace", action="store_true", help="record the per-iteration trace (batched engine)")
    p.add_argument("--shared", type=int, nargs="?", const=1, default=None, metavar="SEED",
                   help="one H and A for the whole batch (q and bounds per problem, drawn from SEED): the stacked form and "
                        "shared_matrices=True alternately; reports both (batched engine on one rank)")
    a = p.parse_args()
    import torch

    world, rank, local_rank = bench.dist_setup("nccl")
    import madqp_jl_amd as M

    mine = M.shard(range(a.batch), rank, world)
    make = lambda be, i: M.DeviceQP.synthetic(be, a.seed + i, a.nx, a.m)
    opts = dict(max_iter=300, step_rule=M.AdaptiveStep(0.995), regularization=M.FixedRegularization(1e-8, -1e-8),
                mu_min=1e-12, driver=a.driver)
    mixed = None
    if a.mixed_patterns is not None and (a.engine != "batched" or world > 1):
        p.error("--mixed-patterns: the batched engine on one rank")
    if a.shared is not None and (a.engine != "batched" or world > 1 or a.mixed_patterns is not None):
        p.error("--shared: the batched engine on one rank, without --mixed-patterns")
    if (a.refine_steps is not None or a.trace) and a.engine != "batched":
        p.error("--refine-steps / --trace: the batched engine")
    if a.engine == "streams":
        M.solve_batch(make, mine[: min(len(mine), a.streams)], local_rank, a.streams, **opts)  # warm-up
        bench.dist_barrier(world)
        t0 = time.perf_counter()
        res = list(M.solve_batch(make, mine, local_rank, a.streams, **opts).values())
        bench.dist_barrier(world)
        dt = bench.max_over_ranks(time.perf_counter() - t0, world, torch.device("cuda", local_rank))
        lockstep = None
    else:
        opts.pop("driver")
        if a.refine_steps is not None:
            opts["refine_steps"] = a.refine_steps
        if a.trace:
            opts["trace"] = True
        be = M.HipBackend(local_rank)
        qps = [make(be, i) for i in mine]  # data generation is not part of the timed solve
        # warm-up with the full batch (a first solver of a given size pays one-time costs -- kernel load, graph
        # instantiation, allocator growth -- that later ones do not: 187 vs 37 ms at 128 problems), then the median
        # of --repeats timed solves, each with a fresh solver: set-up (scaling, start point) + all iterations +
        # read-back are inside the timed region
        legs = {"shared": (qps, {})}
        setup, held = {}, {}
        if a.shared is not None:  # (leg "shared" -- the one bound pattern -- is then the stacked form of the one-model batch)
            stacked, one = one_model(M, qps, a.shared)
            del qps
            legs = {"shared": (stacked, {}), "shared_matrices": (one, dict(shared_matrices=True))}
            setup, held = {k: [] for k in legs}, {k: [] for k in legs}
        if a.mixed_patterns is not None:
            legs["mixed"] = (mixed_patterns(qps, a.mixed_patterns), dict(per_problem_patterns=True))
        for lq, kw in legs.values():
            warm = M.BatchedMPCSolver(lq, be, **kw, **opts)
            warm.solve(check_every=a.check_every)
            warm.close()
        all_times, all_res = {k: [] for k in legs}, {}
        for _ in range(max(1, a.repeats)):
            for leg, (lq, kw) in legs.items():  # (the legs alternate: drifts of the clock or the heat hit both)
                if a.shared is not None:
                    before = held_bytes()
                    tc = time.perf_counter()
                solver = M.BatchedMPCSolver(lq, be, **kw, **opts)
                if a.profile:
                    be.prof_enable(M._lib.PROF_CLASSES)
                    be.prof_reset()
                bench.dist_barrier(world)
                t0 = time.perf_counter()
                if a.shared is not None:  # solve() in its three parts, the set-up timed on its own
                    solver.initialize()
                    torch.cuda.synchronize()
                    setup[leg].append(time.perf_counter() - tc)
                    solver.iterate(check_every=a.check_every)
                    all_res[leg] = solver.results()
                else:
                    all_res[leg] = solver.solve(check_every=a.check_every)
                bench.dist_barrier(world)
                all_times[leg].append(bench.max_over_ranks(time.perf_counter() - t0, world, torch.device("cuda", local_rank)))
                if a.profile and rank == 0:
                    print(leg, {k: (round(v[0], 2), v[1]) for k, v in be.prof_get().items() if v[1]}, flush=True)
                if a.shared is not None:
                    held[leg].append(held_bytes() - before)
                solver.close()
        times, res = all_times["shared"], all_res["shared"]
        dt = sorted(times)[len(times) // 2]
        lockstep = int(max(r["iter"] for r in res))
        mixed = None
        if "mixed" in legs:
            mt, mres = all_times["mixed"], all_res["mixed"]
            mdt = sorted(mt)[len(mt) // 2]
            mit = sum(r["iter"] for r in mres)
            mixed = {"seed": a.mixed_patterns, "QP_per_s": a.batch / mdt, "problem_iterations_per_s": mit / mdt,
                     "solved": sum(r["status"] == M.SOLVE_SUCCEEDED for r in mres),
                     "lock_step_iterations": int(max(r["iter"] for r in mres)), "seconds": mdt, "all_seconds": mt}
    iters = sum(r["iter"] for r in res)
    ok = sum(r["status"] == M.SOLVE_SUCCEEDED for r in res)
    if world > 1:
        import torch.distributed as dist

        t = torch.tensor([iters, ok], dtype=torch.float64, device=torch.device("cuda", local_rank))
        dist.all_reduce(t)
        iters, ok = int(t[0].item()), int(t[1].item())
    if rank == 0:
        extra = {}
        if a.engine == "batched" and a.shared is not None:
            import numpy as np

            med = lambda v: sorted(v)[len(v) // 2]
            st, sh = all_res["shared"], all_res["shared_matrices"]
            same = all(x["status"] == y["status"] and x["iter"] == y["iter"] and x["objective"] == y["objective"] and
                       all(np.array_equal(x[k], y[k]) for k in ("solution", "multipliers", "multipliers_L", "multipliers_U"))
                       for x, y in zip(st, sh))
            sdt = med(all_times["shared_matrices"])
            extra["shared_matrices"] = {
                "seed": a.shared, "bitwise_equal_to_stacked": bool(same),
                "QP_per_s": {"stacked": a.batch / dt, "shared": a.batch / sdt, "ratio": dt / sdt},
                "seconds": {"stacked": times, "shared": all_times["shared_matrices"]},
                "setup_seconds": {"stacked": med(setup["shared"]), "shared": med(setup["shared_matrices"])},
                "solver_device_bytes": {"stacked": med(held["shared"]), "shared": med(held["shared_matrices"])},
                "roofline_shared": batch_roofline(a.nx, a.m, sum(r["iter"] for r in sh), sdt, shared_batch=a.batch)}
        if mixed is not None:
            shared_ips = iters / dt
            extra["mixed_patterns"] = dict(mixed, shared_problem_iterations_per_s=shared_ips,
                                           ratio_problem_iterations_per_s=mixed["problem_iterations_per_s"] / shared_ips)
        print(json.dumps({**extra, "metric": "independent QPs solved per second", "value": a.batch / dt, "unit": "QP/s",
                          "ipm_iterations_per_s": iters / dt, "n_gpus": world, "batch": a.batch,
                          "roofline": batch_roofline(a.nx, a.m, iters, dt),
                          "solved": ok, "config": {"workload": f"{a.batch} x synthetic dense QP nx={a.nx} m={a.m}",
                                                   "engine": a.engine, "streams_per_gpu": a.streams if a.engine == "streams" else None,
                                                   "lock_step_iterations": lockstep,
                                                   "refine_steps": a.refine_steps or 0, "trace": bool(a.trace)},
                          "seconds": dt,
                          "all_seconds": times if a.engine == "batched" else [dt]}), flush=True)


if __name__ == "__main__":
    main()
