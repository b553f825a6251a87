"""CPU (gloo, world_size 2..6): the 2-D block-cyclic distributed Cholesky and its distributed triangular solves
(BASELINE configs[4]).  What runs is the product's own schedule -- madqp_jl_amd/csrc/dist_core.inc,
the file dist.hip compiles for the GPU -- built with CPU loops for the rank-local kernels (tests/csrc/dist_cpu.cpp)
and host-staged collectives over gloo; tiles a rank does not own are NaN-poisoned (tests/dist2d_worker.py)."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def cpuref():
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "tests", "csrc")], stdout=subprocess.DEVNULL)


def test_grid_and_tile_defaults():
    sys.path.insert(0, ROOT)
    from madqp_jl_amd.dist2d import default_grid, default_tile

    assert [default_grid(w) for w in (1, 2, 3, 4, 6, 8)] == [(1, 1), (1, 2), (1, 3), (2, 2), (2, 3), (2, 4)]
    assert default_tile(50000, 8) == 1024 and default_tile(100000, 8) == 1024 and default_tile(5000, 2) == 384
    assert default_tile(300, 4) == 128


MK_UPDATE_COL, MK_POTRF, MK_DIAG_BCAST, MK_TRSM, MK_PACK, MK_EXCHANGE, MK_BULK = 1, 2, 3, 4, 5, 6, 7
ST_U, ST_P = 0, 1


def check_lookahead_order(schedule, p, q, P, Q, T):
    """VERDICT r2 next #1 / ADVICE r2 (medium): on every rank the operand exchange of step k+1 (both broadcast stages,
    stream P) is queued BEFORE the bulk of update k (stream U), and on the ranks of process column (k+1) mod Q the
    whole panel phase of step k+1 -- update of tile column k+1, diagonal tile, panel solve, packing -- precedes both.
    `schedule`: the dop_mark / dop_link sequence recorded by tests/csrc/dist_cpu.cpp from the product's dist_core.inc."""
    pos = {}
    for i, (code, k, st) in enumerate(schedule):
        if code >= 0:
            assert (code, k) not in pos, "every mark once per step"
            pos[(code, k)] = i
            assert st == (ST_P if code in (MK_DIAG_BCAST, MK_EXCHANGE) else ST_U), (code, k, st)

    def linked(a, b, frm, to):  # a link frm -> to issued after position a and before position b
        return any(schedule[i] == [-1, frm, to] for i in range(a + 1, b))

    for k in range(T):
        assert (MK_EXCHANGE, k) in pos, "every rank takes part in every exchange"
    for k in range(T - 1):
        nxt, bulk, xch = k + 1, pos[(MK_BULK, k)], pos[(MK_EXCHANGE, k + 1)]
        assert xch < bulk, f"step {nxt}: operand broadcasts must be queued before the bulk of update {k}"
        assert schedule[xch - 1] == [-1, ST_U, ST_P], "the exchange waits for what U has queued so far"
        first_use = pos.get((MK_UPDATE_COL, k), bulk)
        assert linked(pos[(MK_EXCHANGE, k)], first_use, ST_P, ST_U), f"update {k} must wait for the operands of step {k}"
        if q == nxt % Q:
            upd = pos[(MK_UPDATE_COL, k)]
            chain = [upd]
            if p == nxt % P:
                chain.append(pos[(MK_POTRF, nxt)])
            if P > 1:
                chain.append(pos[(MK_DIAG_BCAST, nxt)])
            if (MK_TRSM, nxt) in pos:
                chain.append(pos[(MK_TRSM, nxt)])
            if Q > 1:
                chain.append(pos[(MK_PACK, nxt)])
            chain += [xch, bulk]
            assert chain == sorted(chain), f"panel phase of step {nxt} out of order on rank ({p},{q}): {chain}"
            if P > 1:  # the panel solve waits for the diagonal tile's broadcast
                assert linked(pos[(MK_DIAG_BCAST, nxt)], chain[chain.index(pos[(MK_DIAG_BCAST, nxt)]) + 1], ST_P, ST_U)
        else:
            assert (MK_UPDATE_COL, k) not in pos and (MK_TRSM, nxt) not in pos and (MK_POTRF, nxt) not in pos


@pytest.mark.parametrize("P,Q,n,nb,group,port", [
    (1, 2, 700, 128, 2, 29541),   # one process row: no transposed broadcast needed beyond the row itself
    (2, 1, 700, 128, 4, 29543),   # one process column
    (2, 2, 1000, 128, 3, 29545),  # partial last tile (1000 = 7*128 + 104), partial last group (8 tiles in groups of 3)
    (2, 3, 900, 256, 1, 29547),   # P and Q coprime, nb = 2 blocks; groups of ONE tile (the per-tile sweeps of round 2)
    (2, 2, 300, 384, 0, 29549),   # fewer tiles than ranks in one direction: some ranks own nothing; default group
    (1, 1, 600, 128, 2, 29551),   # one rank: operands read in place from the factored panel, nothing packed or sent
    (2, 4, 1400, 128, 2, 29553),  # the 8-GPU grid of BASELINE configs[4]: gcd(P, Q) = 2; 11 tiles, 6 groups on 8 ranks
    (2, 2, 1100, 128, 0, 29555),  # default group (4096 rows > n): ONE group, everything collected on rank 0
    (3, 2, 1100, 128, 2, 29557),  # P > Q: a rank's next tile column is several steps away from the panel
    (1, 3, 900, 128, 3, 29559),   # one process row of three: whole-panel factorisation, operands gathered locally
    (4, 1, 800, 128, 2, 29561),   # one process column of four: row operands read in place, column operands stored
])
@pytest.mark.parametrize("bcast", ["collective", "p2p"])
def test_distributed_cholesky_2d(cpuref, tmp_path, P, Q, n, nb, group, port, bcast):
    """`bcast`: every broadcast of the schedule as the library collective (ncclBroadcast in the product; default) or as ONE
    group of point-to-point transfers from the root to each peer of the process row / column / world
    (MADQP_DIST_BCAST=p2p, csrc/dist_core.inc::comm_bcast_p2p: separate xGMI links instead of a ring) -- the
    same schedule, the same buffers, the same results on all eleven grids."""
    world = P * Q
    out = str(tmp_path / "rec")
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", OMP_NUM_THREADS="1", OPENBLAS_NUM_THREADS="1")
    env.pop("MADQP_DIST_GROUP", None)
    env.pop("MADQP_DIST_BCAST", None)
    if bcast == "p2p":
        env["MADQP_DIST_BCAST"] = "p2p"
        port += 100
    if group:
        env["MADQP_DIST_GROUP"] = str(group)
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(world),
           "--master-addr", "127.0.0.1", "--master-port", str(port),
           os.path.join(ROOT, "tests", "dist2d_worker.py"), out, str(P), str(Q), str(n), str(nb)]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    recs = [json.load(open(f"{out}.{k}")) for k in range(world)]
    T = (n + nb - 1) // nb
    assert sum(rec["tiles"] for rec in recs) == T * (T + 1) // 2  # every lower tile has exactly one owner
    for k, rec in enumerate(recs):
        assert (rec["p"], rec["q"]) == (k // Q, k % Q)
        assert rec["spd_info"] == 0 and not rec["nan"]
        assert rec["factor_err"] < 1e-12 and rec["solve_err"] < 1e-11
        assert rec["pad_clean"]  # the zero padding of the local matrix survives (the MFMA kernels read it)
        assert rec["notpd_info"] == rec["notpd_expected"]  # LAPACK's info, identical on every rank
    if world > 1:  # (a single rank has nobody to overlap with: one launch per trailing update, then the next panel)
        for rec in recs:
            check_lookahead_order(rec["schedule"], rec["p"], rec["q"], P, Q, T)
    # the stored operands of the lazy updates are staircases: never more than the full rectangles ld x T nb / ncp x T nb,
    # and with several levels close to the half of them that is ever read (60 -> ~32 GB at C5)
    for rec in recs:
        mm = rec["memory"]
        full_x, full_y = 8 * mm["ld"] * mm["T"] * nb, 8 * mm["ncp"] * mm["T"] * nb
        assert mm["xw"] <= full_x and mm["yw"] <= full_y
        if Q == 1:
            assert mm["xw"] == 0  # row operands read in place from the factored panels
        if world == 1:
            assert mm["xw"] == mm["yw"] == 0 and mm["levels"] == 1
        elif T >= 6:
            lev = mm["levels"]
            assert lev >= 3
            for got, full in ((mm["xw"], full_x), (mm["yw"], full_y)):
                if got:  # (1/2 + 1/(2 levels)) of the rectangle + the 128-row padding of short levels
                    assert got <= full * (0.5 + 0.5 / lev) + 8 * 128 * mm["T"] * nb + 8 * nb * nb * lev, (got, full, lev)
        assert mm["total"] >= mm["K"] + mm["xw"] + mm["yw"]
    # solves: 2 collectives per GROUP and sweep (one reduce of the group's partial sums, one broadcast of its solution)
    G = min(group or max(1, 4096 // nb), T)
    NG = (T + G - 1) // G
    if world > 1 and bcast == "collective":
        assert all(rec["solve_calls"] == {"reduce": 2 * NG, "bcast": 2 * NG} for rec in recs), recs[0]["solve_calls"]
    elif world > 1:  # the solved rows of a group travel point to point: no broadcast call at all, anywhere in the run
        assert all(rec["solve_calls"] == {"reduce": 2 * NG, "bcast": 0} for rec in recs), recs[0]["solve_calls"]
        assert all(rec["calls"]["bcast"] == 0 for rec in recs) and sum(rec["calls"]["send"] for rec in recs) > 0
        assert sum(rec["calls"]["send"] for rec in recs) == sum(rec["calls"]["recv"] for rec in recs)
    # volume: a rank receives each panel tile at most once per operand role; as roots the ranks send
    # (P > 1) T diagonal images + (Q > 1) the row operands + (P > 1) the transposed operands -- never the matrix twice
    total = sum(rec["bytes_sent"] for rec in recs)
    # + the solve groups' diagonal triangles, sent once to their owners (at most G tiles + one diagonal image per step)
    assert total <= 8 * (3 * n * n // 2 + 4 * T * (nb * nb + 2 * 128 * 128 * (nb // 128)) + 64 * T * nb * max(P, Q)
                         + T * (G * nb * nb + nb * nb + 2 * 128 * 128 * (nb // 128)))


def test_a_problem_that_does_not_fit_is_refused_before_anything_is_allocated(cpuref):
    """create computes the per-rank byte total up front and returns MADQP_ERR_ALLOC with the figure
    (madqp_last_error in the product) instead of failing inside the N-th allocation.  CPU build of the same
    dist_core.inc; MADQP_TEST_MEM_FREE stands in for hipMemGetInfo."""
    import ctypes as C
    import textwrap

    code = textwrap.dedent('''
        import ctypes as C, json, os, sys
        lib = C.CDLL(os.path.join(%r, "tests", "_build", "libmadqp_dist_cpuref.so"))
        lib.madqp_distcpu_last_error.restype = C.c_char_p
        h = C.c_void_p()
        rc = lib.madqp_distcpu_create(0, 1, 1, 1, C.c_int64(100000), C.c_int64(1024), None, C.byref(h))
        print(json.dumps(dict(rc=rc, handle=bool(h.value), err=lib.madqp_distcpu_last_error().decode())))
    ''') % ROOT
    env = dict(os.environ, MADQP_TEST_MEM_FREE=str(50 * 10**9))  # 50 GB free; n = 100 000 on one rank needs ~81 GB
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    rec = json.loads(r.stdout.strip().splitlines()[-1])
    assert rec["rc"] == -3 and not rec["handle"]  # MADQP_ERR_ALLOC, nothing handed out
    assert "GB of device memory" in rec["err"] and "50.00 GB are free" in rec["err"], rec["err"]
    need = float(rec["err"].split(" needs ")[1].split(" GB")[0])
    assert 80.0 < need < 81.0, rec["err"]  # the 100 096^2 local matrix alone is 80.15 GB


def test_the_memory_verdict_is_collective(cpuref, tmp_path):
    """byte totals and free memory differ between ranks, and the refusal of a problem that does not
    fit used to be each rank's own -- a rank that fitted went on into the communicator set-up and waited there for
    ever.  Now create() only plans, and allocate() (after the communicators exist) takes ONE collective decision: here
    only rank 1 of a 1 x 2 grid is short of memory, BOTH ranks must return MADQP_ERR_ALLOC -- rank 1 with its own
    figures, rank 0 saying that another rank refused -- and the process group must be usable afterwards."""
    out = str(tmp_path / "rec")
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", OMP_NUM_THREADS="1", OPENBLAS_NUM_THREADS="1",
               MADQP_TEST_SMALL_RANK="1", MADQP_TEST_SMALL_BYTES="100000")
    env.pop("MADQP_TEST_MEM_FREE", None)
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2",
           "--master-addr", "127.0.0.1", "--master-port", "29571",
           os.path.join(ROOT, "tests", "dist2d_refuse_worker.py"), out, "1", "2", "600", "128"]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=300)  # (a hang is the failure this guards)
    assert r.returncode == 0, r.stderr[-3000:]
    recs = [json.load(open(f"{out}.{k}")) for k in range(2)]
    for rec in recs:
        assert rec["rc"] == -3 and not rec["handle"] and rec["comm_error"] is None, rec
        assert rec["rc_again"] == 0, rec
    assert "GB of device memory" in recs[1]["err"] and "are free" in recs[1]["err"], recs[1]["err"]
    assert "other rank(s)" in recs[0]["err"] and "every rank refuses" in recs[0]["err"], recs[0]["err"]


def test_schedule_under_address_and_undefined_sanitizers():
    """tests/csrc_dist/dist_sched_main.cpp: a stand-alone program (never loaded into Python) in which ONE rank walks the
    whole schedule with every collective forced -- operand staircases over several levels, the operand exchange with its
    tile gathers, the band collection with its send-to-self, the group sweeps -- over in-process collectives, under both
    sanitizers.  Per case it factors, solves and holds max|A x - b| / max|b| to 1e-12, or (the case with a negative
    diagonal entry) info to that column; the send queue must be empty at the end."""
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "tests", "csrc_dist")], stdout=subprocess.DEVNULL)
    out = subprocess.run([os.path.join(ROOT, "tests", "_build", "dist_sched_check")], capture_output=True, text=True,
                         timeout=300)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    lines = out.stdout.strip().splitlines()
    assert lines[-1] == "dist schedule ok" and len(lines) == 6 and "FAILED" not in out.stdout, out.stdout
    assert " info 438 " in lines[4] and all(" info 0 " in ln and " queue 0 " in ln for ln in lines[:4]), out.stdout
