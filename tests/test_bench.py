"""CPU: bench.py's bookkeeping (tests/fake_backend.py drives the product's host loop).  The factorisation count of the
timed region must survive the re-initialisations that happen when the solve converges inside it -- round 1 read a
field of the KKT object that initialize() replaces and reported 1 factorisation for 21."""
import bench
import madqp_jl_amd as M
from fake_backend import FakeBackend
from oracle import mpc
from oracle import qp as Q


def make_solver(max_ncorr=0):
    qp = Q.synthetic_qp(20250614, 40, 16)
    dq = M.DeviceQP.from_numpy("cpu", qp.H, qp.q, qp.A, qp.lvar, qp.uvar, qp.lcon, qp.ucon, qp.x0, qp.c0)
    s = M.MPCSolver(dq, FakeBackend(), regularization=M.FixedRegularization(1e-8, -1e-8), max_iter=300,
                    step_rule=M.AdaptiveStep(0.995), mu_min=1e-12, max_ncorr=max_ncorr)
    s.initialize()
    return s


def test_factorizations_counted_across_reinitializations():
    s = make_solver()
    iters = mpc.solve(Q.synthetic_qp(20250614, 40, 16), kkt_system="condensed",
                      regularization=mpc.FixedRegularization(1e-8, -1e-8), step_rule=mpc.AdaptiveStep(0.995),
                      mu_min=1e-12, max_iter=300)["iter"]
    loop = bench.StepLoop(s)
    for _ in range(3):  # warm-up, as bench.measure does
        loop.step()
    loop.reset()
    steps = 3 * iters + 2  # converges (at least) twice inside the timed loop
    totals = []
    for _ in range(steps):
        loop.step()
        totals.append(s.n_factorizations_total)
    assert loop.steps == steps
    assert loop.reinits >= 2
    # one factorisation per iteration plus one start-point factorisation per re-initialisation (no retries here)
    assert loop.factorizations() == steps + loop.reinits
    assert all(b >= a for a, b in zip(totals, totals[1:])), "the counter must be monotone"
    # the object-level counter restarts with every initialize(): this is what bench.py must NOT read
    assert s.kkt.n_factorizations < loop.factorizations()
    assert loop.excluded > 0.0


def test_total_counter_without_reinit_equals_kkt_counter():
    s = make_solver(max_ncorr=3)
    loop = bench.StepLoop(s)
    loop.step()
    loop.step()
    assert loop.reinits == 0 and loop.factorizations() == 2
    assert s.n_factorizations_total == s.kkt.n_factorizations == 3  # start point + 2 iterations


def test_last_resort_reporter_prints_the_held_line_only_when_the_bench_process_dies():
    """bench.py, N > 1: the independent-QPs result is handed to a child process (started before anything touches the
    GPU) before the never-before-run multi-GPU leg starts; if the bench process disappears without saying DONE the
    child prints that line, otherwise nothing -- the run leaves exactly one JSON line either way."""
    import json
    import os
    import subprocess
    import sys
    import textwrap

    code = textwrap.dedent('''
        import json, os, sys
        sys.path.insert(0, %r)
        import bench
        r = bench.LastResortReporter(True)
        r.hold({"metric": "held", "value": 1})
        if sys.argv[1] == "crash":
            os.kill(os.getpid(), 9)
        print(json.dumps({"metric": "real"}), flush=True)
        r.done()
    ''') % os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for mode, expect in (("crash", "held"), ("ok", "real")):
        out = subprocess.run([sys.executable, "-c", code, mode], capture_output=True, text=True, timeout=60)
        lines = [ln for ln in out.stdout.splitlines() if ln.strip()]
        assert len(lines) == 1 and json.loads(lines[0])["metric"] == expect, (mode, out.stdout, out.stderr)


def test_watchdog_measures_silence_not_the_length_of_the_run():
    """one fixed timeout around set-up + warm-up + all steps discards a healthy long run; the watchdog of the
    shared-QP leg is re-armed by every sign of progress and fires only after `seconds` of silence."""
    import time

    fired = []
    dog = bench.Watchdog(0.25, lambda: fired.append(time.perf_counter()))
    t0 = time.perf_counter()
    for _ in range(6):  # 0.6 s of "run", a kick every 0.1 s: longer than the timeout, never silent that long
        time.sleep(0.1)
        dog.kick()
    assert not fired
    time.sleep(0.5)  # silence
    assert len(fired) == 1 and fired[0] - t0 >= 0.6 + 0.25 - 0.05
    dog.stop()
    dog = bench.Watchdog(0.2, lambda: fired.append(0))
    dog.stop()
    time.sleep(0.3)
    assert len(fired) == 1


def test_only_the_json_line_reaches_stdout():
    """The contract is ONE JSON line on stdout, and libraries write there too (RCCL prints a version banner when its
    first communicator comes up -- seen in the forced one-rank run of round 3): after bench.protect_stdout() file
    descriptor 1 is stderr and only bench.emit_json reaches the launcher's stdout."""
    import json
    import os
    import subprocess
    import sys
    import textwrap

    code = textwrap.dedent('''
        import os, sys
        sys.path.insert(0, %r)
        import bench
        bench.protect_stdout()
        os.write(1, b"RCCL version : 2.26.6-HEAD\\n")   # a C library writing to fd 1
        print("a stray print")                             # Python's sys.stdout is fd 1 too
        bench.emit_json({"metric": "x", "value": 1})
    ''') % os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stderr
    lines = [ln for ln in out.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1 and json.loads(lines[0]) == {"metric": "x", "value": 1}, out.stdout
    assert "RCCL version" in out.stderr and "a stray print" in out.stderr


# ---- `python bench.py --gpus N` is a run on N ranks, or no run (VERDICT r3 missing #1) -------------------------------
def test_launch_plan():
    """Round 3 parsed --gpus and never read it: world came from WORLD_SIZE alone, so the un-wrapped `python bench.py
    --gpus 8` ran ONE rank, printed n_gpus: 1 and exited 0."""
    assert bench.launch_plan(1, {}) == ("run", 1)                       # the driver's 1-GPU command
    assert bench.launch_plan(1, {"WORLD_SIZE": "1"}) == ("run", 1)
    assert bench.launch_plan(8, {}) == ("spawn", 8)                     # no launcher: bench.py starts the ranks itself
    assert bench.launch_plan(8, {"WORLD_SIZE": "8", "RANK": "3"}) == ("run", 8)  # the driver's N > 1 command
    for gpus, ws in ((8, "1"), (2, "4"), (1, "2"), (2, "two")):
        plan, why = bench.launch_plan(gpus, {"WORLD_SIZE": ws})
        assert plan == "refuse" and ws in why
    assert bench.launch_plan(0, {})[0] == "refuse"


def _run_bench(argv, env_extra, timeout=600):
    import os
    import subprocess
    import sys

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = {k: v for k, v in os.environ.items()
           if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT", "MADQP_DIST_BACKEND",
                        "MADQP_DIST_SHARE_DEVICE", "MADQP_BENCH_SPAWNED_BY")}
    env.update(PYTHONPATH=os.pathsep.join([os.path.join(root, "tests"), root, env.get("PYTHONPATH", "")]),
               OMP_NUM_THREADS="1", OPENBLAS_NUM_THREADS="1", **env_extra)
    return subprocess.run([sys.executable, os.path.join(root, "bench.py"), *argv], env=env, capture_output=True,
                          text=True, timeout=timeout)


SMALL = ["--steps", "3", "--warmup", "1", "--nx", "40", "--m", "16", "--driver", "python", "--no-cpu-baseline",
         "--extra-timeout", "120"]


def test_gpus_2_without_a_launcher_is_a_run_on_two_ranks():
    """Plain `python bench.py --gpus 2 ...`, no launcher, no GPU: bench.py starts `python -m torch.distributed.run` as a
    child before it imports torch, the two ranks run BOTH legs of the N > 1 protocol over gloo (independent QPs, then the
    shared QP -- here on the test double of tests/bench_double.py, which the line declares), rank 0 prints ONE line, and
    that line says n_gpus: 2 / scaling: strong and carries the communicator size."""
    import json

    p = _run_bench(["--gpus", "2", *SMALL, "--full"], {"MADQP_BENCH_TEST_DOUBLE": "bench_double:Double"})
    assert p.returncode == 0, p.stderr[-3000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, p.stdout
    out = json.loads(lines[0])
    assert out["n_gpus"] == 2 and out["n_gpus_requested"] == 2 and out["scaling"] == "strong"
    assert out["ranks"]["world_size"] == 2 and out["ranks"]["started_by"].startswith("bench.py")
    assert out["comm"]["world_size"] == 2 and out["distributed"]["grid"] == [1, 2]
    assert out["steps"] == 3 and out["value"] > 0 and abs(out["value"] - 3 / (out["ms_per_step"] * 3e-3)) < 1e-6 * out["value"]
    assert out["independent_qps"]["value"] > 0  # the weak-scaling leg, reported beside the headline
    assert "test_double" in out and out["data"].startswith("TEST DOUBLE")  # never mistaken for a measurement
    assert "starting -m torch.distributed.run" in p.stderr


def test_the_drivers_n8_command_is_one_line_on_the_2x4_grid():
    """the one run nobody can rehearse on hardware -- the driver's exact N = 8 form, `python bench.py
    --gpus 8 --steps 20 --warmup 5` (plus a reduced size: this is the scaffolding, not the arithmetic) -- on eight gloo
    ranks of the CPU test double: ONE line, n_gpus 8, the 2 x 4 grid of BASELINE configs[4], communicator sizes 8 / 4 / 2,
    `roofline` present, the independent-QPs leg beside it.  (Eight processes may not share one GPU on this pool -- the box
    allows six -- so the GPU rehearsal, tests/test_gpu_bench.py, runs four ranks on a 2 x 2 grid.)"""
    import json

    p = _run_bench(["--gpus", "8", "--steps", "20", "--warmup", "5", "--nx", "48", "--m", "20", "--driver", "python",
                    "--no-cpu-baseline", "--extra-timeout", "240", "--full"],
                   {"MADQP_BENCH_TEST_DOUBLE": "bench_double:Double"},
                   timeout=900)
    assert p.returncode == 0, p.stderr[-3000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, p.stdout
    out = json.loads(lines[0])
    assert out["n_gpus"] == 8 and out["n_gpus_requested"] == 8 and out["scaling"] == "strong"
    assert out["steps"] == 20 and out["warmup"] == 5 and out["value"] > 0
    assert out["distributed"]["grid"] == [2, 4] and out["config"]["parallelism"].startswith("grid 2x4")
    comm = out["comm"]
    assert (comm["world_size"], comm["row_comm_size"], comm["col_comm_size"]) == (8, 4, 2), comm
    assert out["roofline"]["bound"] == "mfma" and "job_fraction_of_peak" in out["roofline"]
    assert out["independent_qps"]["value"] > 0 and out["ranks"]["world_size"] == 8


def test_world_size_that_differs_from_gpus_is_refused_without_a_line():
    for gpus, env in (("2", {"WORLD_SIZE": "1", "RANK": "0"}), ("2", {"WORLD_SIZE": "4", "RANK": "0"}),
                      ("1", {"WORLD_SIZE": "2", "RANK": "1"})):
        p = _run_bench(["--gpus", gpus, *SMALL], {"MADQP_BENCH_TEST_DOUBLE": "bench_double:Double", **env}, timeout=120)
        assert p.returncode == 2, (p.returncode, p.stderr[-1000:])
        assert p.stdout.strip() == "" and "refused" in p.stderr


def test_one_gpu_line_has_the_reference_rate_definitions():
    """`python bench.py --gpus 1` (the driver's command) stays one process; its line carries `whole_solve`: ONE complete
    solve! with iterations/s = iter / total_time and linear-solver time per factorisation, #factorizations = iter + 1
    (src/solver.jl:353,392; scripts/benchmarks_cpu.jl:52-55)."""
    import json

    p = _run_bench(["--gpus", "1", *SMALL, "--no-second-ncorr", "--full"],
                   {"MADQP_BENCH_TEST_DOUBLE": "bench_double:Double"})
    assert p.returncode == 0, p.stderr[-3000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1
    out = json.loads(lines[0])
    assert out["n_gpus"] == 1 and out["n_gpus_requested"] == 1 and out["scaling"] == "weak"
    assert out["ranks"]["started_by"] == "this process alone" and "comm" not in out
    ws = out["whole_solve"]
    assert ws["solved"] and ws["iter"] > 3 and ws["n_factorizations"] == ws["iter"] + 1
    assert abs(ws["iterations_per_s"] - ws["iter"] / ws["total_time_s"]) < 1e-9 * ws["iterations_per_s"]
    assert ws["total_time_s"] <= ws["wall_s"] + 1e-6
    ref = mpc.solve(Q.synthetic_qp(20250614 + 1, 40, 16), kkt_system="condensed", max_ncorr=3,
                    regularization=mpc.FixedRegularization(1e-8, -1e-8), step_rule=mpc.AdaptiveStep(0.995), mu_min=1e-12,
                    max_iter=300)
    assert ws["iter"] == ref["iter"] and abs(ws["objective"] - ref["objective"]) <= 1e-9 * max(1.0, abs(ref["objective"]))


def test_under_an_external_launcher_the_process_is_one_of_the_ranks():
    """The driver's N > 1 form: `python -m torch.distributed.run --nproc-per-node 2 bench.py --gpus 2 ...` -- WORLD_SIZE
    equals --gpus, nothing is spawned, rank 0 prints the one line and says who started the ranks."""
    import json
    import os
    import subprocess
    import sys

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MADQP_BENCH_SPAWNED_BY")}
    env.update(PYTHONPATH=os.pathsep.join([os.path.join(root, "tests"), root, env.get("PYTHONPATH", "")]),
               OMP_NUM_THREADS="1", OPENBLAS_NUM_THREADS="1", MADQP_BENCH_TEST_DOUBLE="bench_double:Double")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
           "--master-port", "29591", os.path.join(root, "bench.py"), "--gpus", "2", "--steps", "2", "--warmup", "1", "--nx", "40",
           "--ncon", "16", "--driver", "python", "--no-cpu-baseline", "--extra-timeout", "120"]
    p = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-3000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.strip().startswith("{")]
    assert len(lines) == 1, p.stdout
    out = json.loads(lines[0])
    assert out["n_gpus"] == 2 and out["n_gpus_requested"] == 2 and out["scaling"] == "strong"
    assert out["ranks"]["started_by"] == "an external launcher" and out["comm"]["world_size"] == 2


def test_plain_run_is_the_headline_alone_and_dumps_what_the_last_step_computed(tmp_path):
    """`python bench.py --gpus 1 --steps K --warmup W` sets up, warms up, times K steps and prints the line; the legs
    beside the headline are --full's.  --dump-outputs DIR writes what the timed path returns to a caller after its last
    step: the same arguments give the same arrays, and they are those of the solver driven through the same W + K
    steps in this process."""
    import json
    import types

    import numpy as np
    from bench_double import Double

    argv = ["--gpus", "1", "--steps", "4", "--warmup", "2", "--nx", "40", "--m", "16", "--driver", "python"]
    lines, dumps = [], {}
    for run in ("a", "b"):
        p = _run_bench([*argv, "--dump-outputs", str(tmp_path / run)], {"MADQP_BENCH_TEST_DOUBLE": "bench_double:Double"})
        assert p.returncode == 0, p.stderr[-3000:]
        lines = [ln for ln in p.stdout.splitlines() if ln.strip()]
        assert len(lines) == 1, p.stdout
        dumps[run] = {f.stem: np.load(f) for f in (tmp_path / run).glob("*.npy")}
    out = json.loads(lines[0])
    assert out["steps"] == 4 and out["warmup"] == 2 and out["iterations_done"] == 6
    assert abs(out["value"] - 4 / (out["ms_per_step"] * 4e-3)) < 1e-6 * out["value"]
    assert out["unit"] == "iterations/s" and out["higher_is_better"] is True and out["dtype"] == "f64"
    for leg in ("max_ncorr_0", "whole_solve", "value_reference_definition", "extras", "cpu_baseline", "independent_qps"):
        assert leg not in out, leg
    shapes = {"solution": 40, "constraints": 16, "multipliers": 16, "multipliers_L": 40, "multipliers_U": 40, "objective": 1}
    assert {k: v.shape for k, v in dumps["a"].items()} == {k: (n,) for k, n in shapes.items()}
    assert all(v.dtype == np.float64 and np.isfinite(v).all() for v in dumps["a"].values())
    for k in shapes:
        assert np.array_equal(dumps["a"][k], dumps["b"][k]), k

    F = Double()
    be = F.backend(0)
    opts = bench.solver_options(M, types.SimpleNamespace(driver="python", kkt_system="condensed"), 3, "local")
    s = M.MPCSolver(F.local_qp(be, 20250614 + 1, 40, 16), be, **opts)
    s.initialize()
    loop = bench.StepLoop(s)
    for _ in range(6):
        loop.step()
    want = bench.solver_outputs(s)
    for k in shapes:
        np.testing.assert_allclose(dumps["a"][k], want[k], rtol=1e-9, atol=1e-12, err_msg=k)


def test_dump_outputs_samples_long_arrays_at_fixed_positions(tmp_path, monkeypatch):
    import numpy as np

    monkeypatch.setattr(bench, "DUMP_BYTES", 2 * 8 * 100)  # 100 entries per array for two arrays
    outputs = {"long": np.arange(1000, dtype=np.float64), "short": np.arange(7, dtype=np.float64)}
    for run in ("a", "b"):
        bench.dump_outputs(str(tmp_path / run), outputs)
    a, b = np.load(tmp_path / "a" / "long.npy"), np.load(tmp_path / "b" / "long.npy")
    assert a.shape == (100,) and np.array_equal(a, b) and np.all(np.diff(a) > 0)
    assert np.array_equal(np.load(tmp_path / "a" / "short.npy"), outputs["short"])
