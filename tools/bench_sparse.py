#!/usr/bin/env python3
"""Sparse-A front end on a synthetic sparse LP (normal equations) or QP (condensed): time per IPM iteration
and the per-class split.  python tools/bench_sparse.py --nx 60000 --ncon 20000 --per-row 8 --kkt normal

A non-diagonal Hessian, dense against sparse (``DeviceSymCSR``), on the CONT-type problem with a smoothing term on the
controls -- the same command with and without ``--sparse-hessian``:

    python tools/bench_sparse.py --cont 150 --smooth 1.0 --kkt condensed --warmup 2 --steps 5 [--sparse-hessian]

``--bandwidth auto`` (or an integer) runs the assembly and the Cholesky band-limited (option ``kkt_bandwidth``): the CONT-type
normal equations of ``--cont N`` have half-bandwidth 2 N.  The same command without it is the dense schedule to compare with."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def bench_hessian_forms(a, be):
    """Per-iteration cost of one form of a non-diagonal H: iterations/s from a window without the device timers, the
    per-class split (assembly = syrk, the mat-vecs of mul! and eval = gemv) from a second window with them.  Every window
    is the first ``steps`` iterations of a solve started afresh, after a warm-up window of the same kind."""
    import torch

    import madqp_jl_amd as M
    from madqp_jl_amd import preprocess as P

    h = P.boundary_control_qp(a.cont, smooth=a.smooth)
    qp = P.to_device(h, be, sparse_hessian=a.sparse_hessian)
    if isinstance(qp.H, M.DeviceSymCSR):
        form, h_bytes = "csr", sum(t.numel() * t.element_size() for t in (qp.H.ptr, qp.H.col, qp.H.val, qp.H.row))
    else:
        form, h_bytes = "dense", qp.H.numel() * qp.H.element_size()
    kw = {} if a.kkt == "augmented" else dict(regularization=M.FixedRegularization(1e-8, 0.0 if a.kkt == "normal" else -1e-8))
    s = M.MPCSolver(qp, be, kkt_system=a.kkt, driver="native", max_iter=300, kkt_bandwidth=a.bandwidth, kkt_storage=a.storage, **kw)

    def window(steps):  # the first iterations of a fresh solve (the problem converges in a handful): the same ones every time
        s.initialize()
        torch.cuda.synchronize()
        t0, done = time.perf_counter(), 0
        for _ in range(steps):
            if s.iteration_head() is not None:
                break
            s.iteration_body()
            done += 1
        torch.cuda.synchronize()
        return done, time.perf_counter() - t0

    window(a.warmup)
    done, dt = window(a.steps)
    be.prof_enable(M._lib.PROF_CLASSES)
    be.prof_reset()
    pdone, _ = window(a.steps)
    prof = be.prof_get()
    be.prof_enable(())
    split = {c: round(v[0] / max(pdone, 1), 3) for c, v in prof.items() if v[1]}
    print(json.dumps({"workload": f"boundary-control QP N={a.cont} smooth={a.smooth}: nx={h.nvar} m={h.ncon} nnzj={h.nnzj} "
                                  f"nnzh={h.nnzh}, {a.kkt}", "hessian": form, "hessian_bytes": h_bytes,
                      "bandwidth": s.kkt.linear_solver.bandwidth, "iterations_timed": done, "ms_per_iteration": dt / max(done, 1) * 1e3,
                      "iterations_per_s": done / dt if done else None, "iterations_profiled": pdone,
                      "split_ms_per_iteration": split, "assembly_ms": split.get("syrk"), "matvec_ms": split.get("gemv"),
                      "last": s.trace[-1] if s.trace else None}))
    s.close()


def bandwidth_arg(v):
    """--bandwidth: "auto" or a non-negative integer (option kkt_bandwidth)"""
    if v == "auto":
        return v
    if not v.isdigit():
        raise argparse.ArgumentTypeError("auto or a non-negative integer")
    return int(v)


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--nx", type=int, default=60000)
    p.add_argument("--ncon", type=int, default=20000)
    p.add_argument("--per-row", type=int, default=8)
    p.add_argument("--kkt", choices=("normal", "condensed", "augmented"), default="normal")
    p.add_argument("--steps", type=int, default=5)
    p.add_argument("--cont", type=int, default=0, help="N > 0: the CONT-type boundary-control QP on an N x N grid "
                   "(preprocess.boundary_control_qp; N = 300 has the shape of Maros-Meszaros CONT-300), solved to the end")
    p.add_argument("--smooth", type=float, default=0.0, help="with --cont: beta > 0 adds beta h D'D on the controls "
                   "(boundary_control_qp(smooth=beta)): a non-diagonal Hessian, which needs --kkt condensed or augmented; "
                   "the run is then timed per iteration (--warmup iterations, then --steps without and --steps with the "
                   "library's device timers)")
    p.add_argument("--sparse-hessian", action="store_true", help="keep a non-diagonal H sparse (DeviceSymCSR)")
    p.add_argument("--warmup", type=int, default=2)
    p.add_argument("--bandwidth", type=bandwidth_arg, default=None, metavar="{auto,INT}",
                   help="band-limited assembly and Cholesky (kkt_bandwidth); needs a sparse, diagonal or absent Hessian")
    p.add_argument("--storage", choices=("dense", "packed"), default="dense",
                   help="where the band path keeps K (kkt_storage): packed = the band alone; needs --bandwidth")
    a = p.parse_args()
    if a.storage == "packed" and a.bandwidth is None:
        p.error("--storage packed needs --bandwidth")
    import torch

    import madqp_jl_amd as M

    be = M.HipBackend(0)
    if a.cont and a.smooth:
        return bench_hessian_forms(a, be)
    if a.cont:
        from madqp_jl_amd import preprocess as P

        t0 = time.perf_counter()
        h = P.boundary_control_qp(a.cont)
        qp = P.to_device(h, be)
        t_gen = time.perf_counter() - t0
        s = M.MPCSolver(qp, be, kkt_system="normal", regularization=M.FixedRegularization(1e-8, 0.0), driver="native",
                        max_iter=100, kkt_bandwidth=a.bandwidth, kkt_storage=a.storage)
        # two whole solves of the same problem: the first without the device timers (time per iteration), the second
        # with them (the per-class split; a timer scope per launch costs host time the first window must not carry)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = s.solve()
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        be.prof_enable(M._lib.PROF_CLASSES)
        be.prof_reset()
        r2 = s.solve()
        torch.cuda.synchronize()
        prof = be.prof_get()
        be.prof_enable(())
        assert r2["iter"] == r["iter"]
        # the set-up both solves carry, once more on its own: a new KKT object (its storage allocated and zeroed), scaling,
        # starting point; and what the device holds then (the library allocates K beside torch's allocator)
        t0 = time.perf_counter()
        s.initialize()
        torch.cuda.synchronize()
        t_setup = time.perf_counter() - t0
        free, total = torch.cuda.mem_get_info()
        nf = max(r["n_factorizations"], 1)
        print(json.dumps({"workload": f"boundary-control QP N={a.cont}: nx={h.nvar} m={h.ncon} nnz={h.nnzj}, diagonal H, "
                                      "normal equations (m x m dense)", "status": r["status"], "iterations": r["iter"],
                          "bandwidth": s.kkt.linear_solver.bandwidth, "ms_per_iteration": dt / max(r["iter"], 1) * 1e3,
                          "storage": dict(zip(("packed", "ld", "doubles"), be.kkt_storage(s.kkt._h))),
                          "setup_seconds": t_setup, "device_bytes_in_use": total - free,
                          "ld_pad": os.environ.get("MADQP_BAND_LD_PAD"),
                          "objective": r["objective"], "solve_seconds": dt, "generate_seconds": t_gen,
                          "factorizations": r["n_factorizations"], "band_w": os.environ.get("MADQP_CHOL_BAND_W"),
                          "sweep_band": os.environ.get("MADQP_SWEEP_BAND"),
                          "sweep_band_blocks": s.kkt.linear_solver.sweep_band_blocks,
                          "ms_per_factorization": {c: round(v[0] / nf, 2) for c, v in prof.items() if v[1]},
                          "last": r["trace"][-1]}))
        s.close()
        return
    rng = np.random.default_rng(7)
    m, n, k = a.ncon, a.nx, a.per_row
    rows = np.repeat(np.arange(m), k + 1)
    cols = np.concatenate([rng.integers(0, n, size=(m, k)), (np.arange(m) % n)[:, None]], axis=1).ravel()
    key = np.unique(rows * n + cols)  # drop duplicates
    rows, cols = key // n, key % n
    csr = M.DeviceCSR(be.device, m, n, rows, cols, rng.standard_normal(len(rows)))
    f64 = dict(dtype=torch.float64, device=be.device)
    z = lambda c, v: torch.full((c,), v, **f64)
    q = torch.as_tensor(rng.standard_normal(n), **f64)
    H = None
    if a.kkt == "condensed":
        H = torch.empty((n, n), **f64)
        be.gen_wigner(M.stream_key(11, 2), n, 1.0 / np.sqrt(n), H)
    qp = M.DeviceQP(H, q, csr, z(n, 0.0), z(n, 1.0), z(m, 0.0), z(m, 1.0), z(n, 0.0))
    reg = M.FixedRegularization(1e-8, 0.0 if a.kkt == "normal" else -1e-8)
    s = M.MPCSolver(qp, be, kkt_system=a.kkt, regularization=reg, driver="native", max_iter=300, kkt_bandwidth=a.bandwidth, kkt_storage=a.storage)
    s.initialize()
    s.iteration_head()
    s.iteration_body()
    be.prof_enable(M._lib.PROF_CLASSES)
    be.prof_reset()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    done = 0
    for _ in range(a.steps):
        if s.iteration_head() is not None:
            break
        s.iteration_body()
        done += 1
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    prof = be.prof_get()
    print(json.dumps({"workload": f"sparse {a.kkt} nx={n} m={m} nnz={csr.nnz}", "ms_per_iteration": dt / max(done, 1) * 1e3,
                      "iterations": done, "split_ms_per_iteration": {c: round(v[0] / max(done, 1), 3) for c, v in prof.items() if v[1]},
                      "last": s.trace[-1] if s.trace else None}))
    s.close()


if __name__ == "__main__":
    main()
