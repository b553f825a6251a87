"""Measures ``madqp_chol_solve_many``: the forced column-by-column path against the forced blocked path on the same seeded
block of right-hand sides, for nrhs = 1 .. 128, on four factors -- one GPU command, one process:

    python tools/bench_solve_many.py --out profiles/solve_many.json

Cases: n = 5 000 and n = 12 800 in the padded layout (the mid-size schedule, U = L' present), n = 50 000 in the unpadded
layout (the left-looking schedule; the 20 GB factor fits), and a band matrix of the CONT-300 shape (order 90 000,
half-bandwidth 600: the normal equations of ``tools/bench_sparse.py --cont 300``) in packed storage.  The dense matrices are
``madqp_gen_wigner`` (Wigner + 3 I); the band matrix is strictly diagonally dominant, generated on the device from a seed.

Per cell: every shape is warmed up, then windows of at least ``--window`` seconds between device events, the two paths
alternating, ``--repeats`` windows each; the median and the spread (max - min) of the per-call time are reported.  Every
timed call solves a fresh copy of the block (the device copy is inside the window, for both paths alike).  With each
time: the launches and the factor bytes of the info call, bytes / time against 8 TB/s, the time per launch, and the largest
column-wise relative difference between the two paths.  ``min_nrhs``: the smallest measured nrhs from which on the blocked
median beats the looped one by more than the spread in every case -- the default written into chol.hip.

``--kkt`` measures ``madqp_kkt_solve_many`` instead, with block products (``madqp_kkt_set_block_products``) off and on,
alternating in the same windows, for nrhs = 2 .. 128 and 0 and 1 refinement steps, on the dense condensed and the dense
normal object at n_x = 5 000, m = 2 000 (one seeded A) and the packed-band normal equations of
``tools/bench_sparse.py --cont N`` (``--cont``, default 300):

    python tools/bench_solve_many.py --kkt --out profiles/kkt_many.json

``--tiny`` runs the same program on small shapes (a rehearsal of the tool, not a measurement).  No GPU: the tool fails."""
import argparse
import json
import math
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import madqp_jl_amd as M  # noqa: E402

NRHS = (1, 2, 4, 8, 16, 32, 64, 128)
HBM_BYTES_PER_S = 8e12
FAR = 1 << 30  # min_nrhs that forces the column-by-column path


def dense_case(be, n, padded):
    npad = (n + 127) // 128 * 128
    lda = npad + 2 if padded else n + 2
    K = torch.empty((n, lda), dtype=torch.float64, device=be.device)
    be.gen_wigner(M.stream_key(20, 2), n, 1.0 / math.sqrt(n), K)
    h = be.chol_create(n)
    assert be.chol_factor(h, K, lda) == 0
    return h, K


def band_case(be, n, bw):
    """packed storage: entry (i, j) at P[i + j ld] = AB[j, i - j] with AB of row length ld + 1"""
    h = be.chol_create(n)
    be.chol_set_bandwidth(h, bw)
    ld, doubles = be.chol_packed_layout(h)
    be.chol_set_packed(h, True)
    P = torch.zeros(doubles, dtype=torch.float64, device=be.device)
    gen = torch.Generator(device=be.device)
    gen.manual_seed(20)
    AB = P[: n * (ld + 1)].view(n, ld + 1)
    AB[:, 1: bw + 1] = (2.0 * torch.rand((n, bw), dtype=torch.float64, device=be.device, generator=gen) - 1.0) / bw
    j = torch.arange(n, device=be.device).unsqueeze(1)
    d = torch.arange(1, bw + 1, device=be.device).unsqueeze(0)
    AB[:, 1: bw + 1] *= (j + d < n)  # rows beyond the order hold nothing
    AB[:, 0] = 3.0  # the off-diagonal row sums stay below 2: strictly diagonally dominant
    assert be.chol_factor(h, P, ld) == 0
    return h, P


def window(be, h, B0, B, reps):
    """ms per call over `reps` calls of copy + solve between two device events"""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        B.copy_(B0)
        be.chol_solve_many(h, B, B.shape[1])
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / reps


def measure(be, name, h, n, seconds, repeats, has_upper):
    cells = []
    for nrhs in NRHS:
        B0 = torch.empty((nrhs, n), dtype=torch.float64, device=be.device)
        be.gen_normal(M.stream_key(21, nrhs), 0, B0)
        B = torch.empty_like(B0)
        paths = {"looped": FAR, "blocked": 2}
        out, info, reps, times = {}, {}, {}, {"looped": [], "blocked": []}
        for p, mn in paths.items():
            if p == "blocked" and nrhs == 1:
                continue  # one right-hand side is madqp_chol_solve itself
            be.chol_set_solve_many_min(h, mn)
            info[p] = be.chol_solve_many_info(h, nrhs)
            window(be, h, B0, B, 2)  # warm-up of the shape (tile tables, workspace)
            out[p] = B.clone()
            reps[p] = max(1, math.ceil(seconds * 1e3 / window(be, h, B0, B, 2)))
        for _ in range(repeats):  # alternating
            for p in times:
                if p in reps:
                    be.chol_set_solve_many_min(h, paths[p])
                    times[p].append(window(be, h, B0, B, reps[p]))
        cell = {"nrhs": nrhs}
        for p in times:
            if p not in reps:
                continue
            t = np.array(times[p])
            med = float(np.median(t))
            cell[p] = {"ms_median": med, "ms_min": float(t.min()), "ms_max": float(t.max()), "ms_spread": float(t.max() - t.min()),
                       "calls_per_window": reps[p], "path": info[p][0], "launches": info[p][1], "factor_bytes": info[p][3],
                       "fraction_of_8TBps": info[p][3] / (med * 1e-3) / HBM_BYTES_PER_S,
                       "us_per_launch": med * 1e3 / max(info[p][1], 1)}
        if "blocked" in out:
            a, b = out["looped"], out["blocked"]
            cell["max_rel_diff"] = float(((a - b).norm(dim=1) / a.norm(dim=1)).max())
            cell["speedup"] = cell["looped"]["ms_median"] / cell["blocked"]["ms_median"]
        cells.append(cell)
        print(f"{name} nrhs={nrhs}: " + ", ".join(f"{p} {cell[p]['ms_median']:.3f} ms (spread {cell[p]['ms_spread']:.3f})"
                                                   for p in ("looped", "blocked") if p in cell), flush=True)
    ws = be.chol_solve_many_info(h, 128)[2]
    return {"case": name, "n": n, "has_upper": has_upper, "workspace_doubles": ws, "cells": cells}


def cutover(cases):
    """smallest measured nrhs from which on blocked beats looped by more than the spread, in every case; None: never"""
    good = {}
    for nrhs in NRHS[1:]:
        good[nrhs] = True
        for c in cases:
            cell = next(x for x in c["cells"] if x["nrhs"] == nrhs)
            lo, bl = cell["looped"], cell["blocked"]
            good[nrhs] &= lo["ms_median"] - bl["ms_median"] > max(lo["ms_spread"], bl["ms_spread"])
    best = None
    for nrhs in reversed(NRHS[1:]):
        if not good[nrhs]:
            break
        best = nrhs
    return best


# ---- --kkt: madqp_kkt_solve_many with block products off and on ------------------------------------------------------------
def seed_state(be, st, seed):
    """iterates well inside their bounds, multipliers of order one (the state of tests/test_gpu_solve_many.py)"""
    gen = torch.Generator(device=be.device)
    gen.manual_seed(seed)
    rnd = lambda k: torch.rand(k, dtype=torch.float64, device=be.device, generator=gen)
    x = torch.randn(st.n, dtype=torch.float64, device=be.device, generator=gen)
    st.x.copy_(x)
    st.xl.copy_(x - (0.5 + rnd(st.n)))
    st.xu.copy_(x + (0.5 + rnd(st.n)))
    st.zl.copy_(0.3 + rnd(st.n))
    st.zu.copy_(0.3 + rnd(st.n))
    st.y.copy_(torch.randn(st.m, dtype=torch.float64, device=be.device, generator=gen))


def dense_kkt_case(be, form, nx, m):
    """(object, keep-alive) of the dense condensed or normal form on one seeded A; every row an inequality, every slack and
    half of the variables bounded"""
    A = torch.empty((m, nx), dtype=torch.float64, device=be.device)
    be.gen_normal(M.stream_key(22, 0), 0, A)
    A *= 1.0 / math.sqrt(nx)
    lb = list(range(0, nx, 2)) + list(range(nx, nx + m))
    ub = list(range(1, nx, 3)) + list(range(nx, nx + m))
    st = be.new_state(nx + m, m, lb, ub)
    if form == "condensed":
        H = torch.empty((nx, nx), dtype=torch.float64, device=be.device)
        be.gen_wigner(M.stream_key(22, 1), nx, 1.0 / math.sqrt(nx), H)
        kkt, keep, del_c = M.HIPCondensedKKTSystem(be, st, nx, list(range(m)), H, A), (H, A), -1.0
    else:
        At = A.T.contiguous()
        kkt, keep, del_c = M.HIPNormalKKTSystem(be, st, nx, list(range(m)), None, At), (At,), 0.0
    kkt.initialize()
    seed_state(be, st, 23)
    kkt.set_aug_diagonal_reg(1.0, del_c)
    kkt.factorize_wrapper()
    assert kkt.linear_solver.is_factorized()
    return kkt, keep


def sparse_kkt_case(be, cont):
    """the packed-band normal equations of ``tools/bench_sparse.py --cont N`` after the first iteration of a solve: the
    driver's own object, state and factor"""
    from madqp_jl_amd import preprocess as P

    qp = P.to_device(P.boundary_control_qp(cont), be)
    s = M.MPCSolver(qp, be, kkt_system="normal", regularization=M.FixedRegularization(1e-8, 0.0), driver="native", max_iter=1,
                    kkt_bandwidth="auto", kkt_storage="packed")
    s.solve()
    assert s.kkt.linear_solver.is_factorized()
    return s.kkt, (s, qp)


def kkt_window(kkt, W0, W, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        W.copy_(W0)
        kkt.solve_many(W)
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / reps


def measure_kkt(be, name, kkt, seconds, repeats, refine):
    st = kkt.st
    ntot = st.n + st.m + st.nlb + st.nub
    kkt.set_refine(refine)
    cells = []
    for nrhs in NRHS[1:]:
        W0 = torch.empty((nrhs, ntot), dtype=torch.float64, device=be.device)
        be.gen_normal(M.stream_key(24, nrhs), 0, W0)
        W = torch.empty_like(W0)
        modes = {"loop": False, "block": True}
        out, info, reps, times = {}, {}, {}, {"loop": [], "block": []}
        for p, on in modes.items():
            kkt.set_block_products(on)
            kkt_window(kkt, W0, W, 2)  # warm-up of the shape (workspace, tile tables)
            info[p] = be.kkt_many_info(kkt._h, nrhs)
            out[p] = W.clone()
            reps[p] = max(1, math.ceil(seconds * 1e3 / kkt_window(kkt, W0, W, 2)))
        for _ in range(repeats):  # alternating
            for p, on in modes.items():
                kkt.set_block_products(on)
                times[p].append(kkt_window(kkt, W0, W, reps[p]))
        cell = {"nrhs": nrhs}
        for p in modes:
            t = np.array(times[p])
            cell[p] = {"ms_median": float(np.median(t)), "ms_min": float(t.min()), "ms_max": float(t.max()),
                       "ms_spread": float(t.max() - t.min()), "calls_per_window": reps[p], "path": info[p][0],
                       "passes_over_A": info[p][1], "passes_over_H": info[p][2], "workspace_doubles": info[p][3]}
        cell["max_rel_diff"] = float(((out["loop"] - out["block"]).norm(dim=1) / out["loop"].norm(dim=1)).max())
        cell["speedup"] = cell["loop"]["ms_median"] / cell["block"]["ms_median"]
        cells.append(cell)
        print(f"{name} refine={refine} nrhs={nrhs}: " + ", ".join(f"{p} {cell[p]['ms_median']:.3f} ms (spread {cell[p]['ms_spread']:.3f})"
                                                                   for p in modes) + f", loop / block {cell['speedup']:.2f}", flush=True)
    kkt.set_block_products(False)
    kkt.set_refine(0)
    # the crossing point: the smallest measured nrhs from which on block beats loop by more than the spread; None: never
    cross = None
    for cell in reversed(cells):
        if cell["loop"]["ms_median"] - cell["block"]["ms_median"] <= max(cell["loop"]["ms_spread"], cell["block"]["ms_spread"]):
            break
        cross = cell["nrhs"]
    return {"case": name, "ntot": ntot, "refine": refine, "block_wins_from": cross, "cells": cells}


def main_kkt(a, be):
    nx, m, cont = (600, 250, 12) if a.tiny else (5000, 2000, a.cont)
    cases = []
    for name, make in ((f"dense-condensed-{nx}x{m}", lambda: dense_kkt_case(be, "condensed", nx, m)),
                       (f"dense-normal-{nx}x{m}", lambda: dense_kkt_case(be, "normal", nx, m)),
                       (f"sparse-normal-packed-cont{cont}", lambda: sparse_kkt_case(be, cont))):
        kkt, keep = make()
        for refine in (0, 1):
            cases.append(measure_kkt(be, name, kkt, a.window, a.repeats, refine))
        if not name.startswith("sparse"):
            kkt.close()  # (the sparse object is its driver's)
        del kkt, keep
        torch.cuda.empty_cache()
    res = {"tool": "tools/bench_solve_many.py --kkt", "device": torch.cuda.get_device_name(0), "tiny": a.tiny,
           "window_s": a.window, "repeats": a.repeats, "cases": cases}
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")
    print(json.dumps([{k: v for k, v in c.items() if k != "cells"} for c in cases]))
    be.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="write the JSON here (default: stdout only)")
    ap.add_argument("--window", type=float, default=0.5, help="seconds per timed window")
    ap.add_argument("--repeats", type=int, default=3, help="windows per path and cell")
    ap.add_argument("--tiny", action="store_true", help="small shapes: a rehearsal of the tool, not a measurement")
    ap.add_argument("--kkt", action="store_true", help="madqp_kkt_solve_many with block products off and on (-> profiles/kkt_many.json)")
    ap.add_argument("--cont", type=int, default=300, help="with --kkt: the N of the boundary-control QP of the sparse case")
    a = ap.parse_args()
    be = M.HipBackend(0)
    if a.kkt:
        return main_kkt(a, be)
    shapes = [("mid-5000-padded", 5000, True), ("mid-12800-padded", 12800, True), ("large-50000-unpadded", 50000, False)]
    band = ("band-90000-bw600-packed", 90000, 600)
    if a.tiny:
        shapes = [("mid-600-padded", 600, True), ("left-700-unpadded", 700, False)]
        band = ("band-1537-bw300-packed", 1537, 300)
    cases = []
    for name, n, padded in shapes:
        h, K = dense_case(be, n, padded)
        cases.append(measure(be, name, h, n, a.window, a.repeats, has_upper=padded))
        be.chol_destroy(h)
        del K
        torch.cuda.empty_cache()
    h, P = band_case(be, band[1], band[2])
    cases.append(measure(be, band[0], h, band[1], a.window, a.repeats, has_upper=False))
    be.chol_destroy(h)
    res = {"tool": "tools/bench_solve_many.py", "device": torch.cuda.get_device_name(0), "tiny": a.tiny, "window_s": a.window,
           "repeats": a.repeats, "min_nrhs": cutover(cases), "cases": cases}
    text = json.dumps(res, indent=1)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")
    print(json.dumps({k: v for k, v in res.items() if k != "cases"}))
    be.close()


if __name__ == "__main__":
    main()
