#!/usr/bin/env python3
"""How far the lock-step batched engine is from the LAPACK oracle PER ITERATION, case by case, in units of the CPU noise floor
(tests/parity.py: ensemble_floor) -- with and without a refinement step.  TEST TOOLING (imports oracle/ and tests/); needs a GPU.

The soak streams the batched engine runs in tests/test_gpu_soak.py, (9000, 200, LPs) and (1000, 150), plus (31000, 400, LPs),
each problem as a batch of one with trace=True, under three settings:
    refine0        refine_steps = 0 (the engine's default)
    refine1        refine_steps = 1
    refine0_full   refine_steps = 0 with MADQP_BATCH_INCR=0 (model evaluated from scratch every iteration)
The knob is read once per process, so every setting runs in a child process of its own, under its own time limit; the first
child that fails ends the run.  The oracle's runs and the floors are computed once, on the CPU, before any child starts.

    python tools/parity_table_batched.py --out profiles/batched_parity_ratios.json [--soak-count N] [--timeout S]

Ratios are formed only where the stated bar (1e-9 / 1e-6 per iteration, 1e-7 in x, 1e-9 in the objective) is exceeded;
0 = within the bar.  A case whose iteration count differs from the oracle's has no ratio: it is listed as a tie / mismatch."""
import argparse
import json
import os
import pickle
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import parity  # noqa: E402
import parity_table  # noqa: E402  (case builder and the CPU side of a case)

STREAMS = ((9000, 200, True), (1000, 150, False), (31000, 400, True))
SETTINGS = {"refine0": (0, {}), "refine1": (1, {}), "refine0_full": (0, {"MADQP_BATCH_INCR": "0"})}
THRESHOLDS = (1, 2, 4, 16)


def make_cases(soak_count):
    from test_gpu_soak import soak_cases

    for seed0, count, only_lp in STREAMS:
        for k, (seed, n, m, lp) in enumerate(soak_cases(seed0, count, only_lp)):
            if k < soak_count:
                yield f"soak{seed}{'_lp' if lp else ''}", ("random", seed, n, m, lp), {}


def child(setting, cpu_file, rows_file, soak_count):
    """One setting through the batched engine (this process is the only one that opens the GPU)."""
    import madqp_jl_amd as M

    refine, env = SETTINGS[setting]
    assert all(os.environ.get(k) == v for k, v in env.items()), "the parent sets the environment of a setting"
    cpu = pickle.load(open(cpu_file, "rb"))
    be = M.HipBackend(0)
    REG = M.FixedRegularization(1e-8, -1e-8)
    rows = {}
    for name, spec, _ in make_cases(soak_count):
        c = cpu[name]
        if c is None:
            continue
        qp = parity_table.build(spec)
        dq = M.DeviceQP.from_numpy(be.device, qp.H, qp.q, qp.A, qp.lvar, qp.uvar, qp.lcon, qp.ucon, qp.x0, qp.c0)
        s = M.BatchedMPCSolver([dq], be, regularization=REG, refine_steps=refine, trace=True)
        r = s.solve()[0]
        s.close()
        if r["status"] != c["ref"]["status"]:
            rows[name] = dict(status=int(r["status"]))
            continue
        row = dict(iter=int(r["iter"]), mean_residual_ratio=float(np.mean([t["residual_ratio"] for t in r["trace"]])))
        if r["iter"] != c["ref"]["iter"]:
            try:
                row["tie"] = parity.iteration_parity(r, c["ref"], 1e-8, name, lp=spec[4]) == "tie"
            except AssertionError:
                row["tie"] = False
        else:
            row["vs_ensemble"] = parity.ratios_to_floor(r, c["ref"], c["floor"])
        rows[name] = row
    be.close()
    json.dump(rows, open(rows_file, "w"), default=float)


def summary(rows, key):
    have = [(max(r[key]["vs_ensemble"].values()), r["case"]) for r in rows if r.get(key, {}).get("vs_ensemble")]
    v = np.array([x for x, _ in have]) if have else np.zeros(1)
    ties = [r["case"] for r in rows if r.get(key, {}).get("tie") is True]
    bad = [r["case"] for r in rows if key in r and (r[key].get("tie") is False or "status" in r[key])]
    worst = max(have) if have else (0.0, None)
    return dict(cases=len(have), threshold_ties=ties, other_mismatches=bad, worst=float(worst[0]), worst_case=worst[1],
                **{f"over_{t}": int((v > t).sum()) for t in THRESHOLDS})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "batched_parity_ratios.json"))
    ap.add_argument("--soak-count", type=int, default=1000, help="cases per soak stream")
    ap.add_argument("--workers", type=int, default=min(16, os.cpu_count() or 1))
    ap.add_argument("--timeout", type=int, default=300, help="seconds per setting (child process)")
    ap.add_argument("--child", nargs=3, metavar=("SETTING", "CPU_FILE", "ROWS_FILE"), help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        return child(*a.child, a.soak_count)
    from concurrent.futures import ProcessPoolExecutor

    cases = list(make_cases(a.soak_count))
    t0 = time.time()
    # (one BLAS thread per worker: the problems have order <= 260, and `workers` processes with a thread pool each only
    # get in each other's way; the workers are spawned, so they read the setting when they import numpy)
    import multiprocessing

    saved = {k: os.environ.get(k) for k in ("OMP_NUM_THREADS", "OPENBLAS_NUM_THREADS", "MKL_NUM_THREADS")}
    os.environ.update({k: "1" for k in saved})
    try:
        with ProcessPoolExecutor(a.workers, mp_context=multiprocessing.get_context("spawn")) as ex:
            cpu = dict(ex.map(parity_table.cpu_side, cases, chunksize=4))
    finally:
        for k, v in saved.items():
            os.environ.pop(k) if v is None else os.environ.__setitem__(k, v)
    print(f"[parity_table_batched] {len(cases)} cases, CPU side {time.time() - t0:.0f} s", file=sys.stderr, flush=True)
    per_setting = {}
    with tempfile.TemporaryDirectory() as tmp:
        cpu_file = os.path.join(tmp, "cpu.pkl")
        pickle.dump(cpu, open(cpu_file, "wb"))
        for setting, (_, env) in SETTINGS.items():  # a fresh child per setting; stop at the first one that fails
            rows_file = os.path.join(tmp, setting + ".json")
            t1 = time.time()
            subprocess.run([sys.executable, os.path.abspath(__file__), "--soak-count", str(a.soak_count), "--child", setting,
                            cpu_file, rows_file], env={**os.environ, **env}, timeout=a.timeout, check=True)
            per_setting[setting] = json.load(open(rows_file))
            print(f"[parity_table_batched] {setting}: {time.time() - t1:.0f} s", file=sys.stderr, flush=True)
    rows = []
    for name, spec, _ in cases:
        c = cpu[name]
        if c is None:
            continue
        row = dict(case=name, n=spec[2], m=spec[3], lp=bool(spec[4]), iter_ref=c["ref"]["iter"], floor_dx=c["floor"]["dx"],
                   ensemble_stopped_elsewhere=c["floor"]["stopped_elsewhere"])
        for setting in SETTINGS:
            if name in per_setting[setting]:
                row[setting] = per_setting[setting][name]
        rows.append(row)
    out = dict(what="batched engine (batches of one, trace=True) distance from the LAPACK oracle per iteration / in x / in the "
                    "objective, in units of the CPU noise floor (ensemble of five valid executions); 0 = within the stated bar",
               streams=[dict(seed0=s, count=c, only_lp=o) for s, c, o in STREAMS],
               settings={k: dict(refine_steps=v[0], env=v[1]) for k, v in SETTINGS.items()},
               summary={k: summary(rows, k) for k in SETTINGS}, rows=rows)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    open(a.out, "w").write(json.dumps(out, indent=1, default=float))
    print(json.dumps(out["summary"], indent=1))


if __name__ == "__main__":
    main()
