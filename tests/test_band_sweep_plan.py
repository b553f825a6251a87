"""CPU: the job lists of the triangular sweeps under a band (madqp_jl_amd/csrc/band_plan.inc: band_sweep_blocks,
band_sweep_jobs; compiled for the CPU by tests/csrc_band).  The lists are checked against the tiles of the band, the
waits of the kernels and the extent of the factorisation's plan; both sweeps are executed in numpy along the lists, with
partial sums per job and the owner's sum over them, on factors that hold NaN wherever the sweeps must not read.  The kernels
that run the lists are held in tests/test_gpu_band_sweeps.py."""
import os
import subprocess

import numpy as np
import pytest
import scipy.linalg as sla

from band_cases import NB, ROOT, band_lib, band_spd, dense_jobs, plan, ranges, sweep_jobs

NS = (1, 128, 129, 500, 1537, 2100, 9000)
CHUNKS = (1, 2, 3, 5, 64)
SHAPES = [(n, bw) for n in NS for bw in sorted({0, 1, 127, 128, 129, 300, 640, n - 1}) if bw < n]


@pytest.mark.parametrize("n,bw", SHAPES)
def test_jobs_cover_the_band_once(n, bw):
    lib = band_lib()
    nblk = max(1, (n + NB - 1) // NB)
    kb = lib.band_sweep_blocks_c(bw)
    assert kb == (bw + 127) // 128
    reach = lib.band_sweep_reach_c(n, kb)
    assert reach == min(n - 1, kb * 128 + 127)
    extent = plan(n, bw)[1]
    assert reach <= extent, "the sweeps stay inside the extent of the factorisation"
    for chunk in CHUNKS:
        jobs, maxc = sweep_jobs(nblk, kb, chunk)
        assert maxc == max(1, (nblk - 1 + chunk - 1) // chunk)
        assert jobs == sorted(jobs) and len(set(jobs)) == len(jobs), "ascending in (r, c)"
        ticket = {job: t for t, job in enumerate(jobs)}
        seen = np.zeros((nblk, nblk), dtype=np.int64)
        owners = np.zeros(nblk, dtype=np.int64)
        for t, (r, c) in enumerate(jobs):
            assert 0 <= r < nblk and 0 <= c < maxc and r * maxc + c < nblk * maxc, "the slot exists"
            j0, j1, owner, clo = ranges(r, c, kb, chunk)
            assert j0 <= j1
            seen[r, j0:j1] += 1
            assert all(ticket[(j, max(1, (j + chunk - 1) // chunk) - 1)] < t for j in range(j0, j1)), \
                "a job polls solution blocks of earlier tickets only"
            if owner:
                owners[r] += 1
                for cc in range(clo, c):
                    assert (r, cc) in ticket and ticket[(r, cc)] < t, "the owner waits for emitted, earlier jobs only"
                    assert not ranges(r, cc, kb, chunk)[2]
        r, j = np.indices((nblk, nblk))
        assert np.array_equal(seen, ((j >= np.maximum(0, r - kb)) & (j < r)).astype(np.int64)), \
            "every tile of the band in exactly one job, no other tile in any"
        assert np.all(owners == 1), "every row has its owner, the rows without tiles too"
        if kb >= nblk - 1:
            assert jobs == dense_jobs(nblk, chunk)
        assert sweep_jobs(nblk, -1, chunk)[0] == dense_jobs(nblk, chunk)
        if bw == n - 1:
            assert jobs == dense_jobs(nblk, chunk), "full bandwidth: the dense list"


def test_band_jobs_are_few():
    """order 90 000, bw 600 (CONT-300): 5 tiles per row instead of up to 703.  One job per row at the default chunk,
    except the 4 rows behind each of the 10 chunk boundaries whose 5 tiles straddle it: 704 + 40 jobs; the dense list has
    1 + 64 (1 + .. + 10) + 63 * 11."""
    nblk = (90000 + NB - 1) // NB
    jobs, maxc = sweep_jobs(nblk, 5, 64)
    assert nblk == 704 and len(jobs) == 704 + 4 * 10 and maxc == 11
    assert len(dense_jobs(nblk, 64)) == 1 + 64 * 55 + 63 * 11 == 4214


def reference(n, bw):
    """(L, b, x): the scipy factor of band_spd(n, bw), a right-hand side, cho_solve.  Not cached: every (n, bw) is used
    once, and at n = 9000 one factor is 648 MB."""
    K = band_spd(n, bw)
    L = sla.cholesky(K, lower=True, overwrite_a=True, check_finite=False)
    del K
    b = np.random.default_rng(n + bw).standard_normal(n)
    return L, b, sla.cho_solve((L, True), b, check_finite=False)


def run_sweep(W, b, n, kb, chunk, backward):
    """One sweep along the job list on the stored factor W, block by block as the kernels go: partial sums per job,
    filed under (row of the chain, chunk); the owner adds those from its first chunk on, then solves its diagonal block."""
    nblk = max(1, (n + NB - 1) // NB)
    jobs, _ = sweep_jobs(nblk, kb, chunk)
    blk = lambda k: slice(k * NB, min(n, (k + 1) * NB))
    x = np.full(n, np.nan)
    part = {}
    for rr, c in jobs:
        j0, j1, owner, clo = ranges(rr, c, kb, chunk)
        r = nblk - 1 - rr if backward else rr  # the block of the matrix
        acc = np.zeros(blk(r).stop - blk(r).start)
        for k in range(j0, j1):
            j = nblk - 1 - k if backward else k  # source block
            acc += (W[blk(j), blk(r)].T if backward else W[blk(r), blk(j)]) @ x[blk(j)]
        if not owner:
            part[(rr, c)] = acc
            continue
        far = np.zeros_like(acc)
        for cc in range(clo, c):
            far += part[(rr, cc)]
        D = np.tril(W[blk(r), blk(r)])
        x[blk(r)] = sla.solve_triangular(D, b[blk(r)] - (far + acc), lower=True, trans=1 if backward else 0)
    return x


@pytest.mark.parametrize("n,bw", SHAPES)
def test_executed_sweeps_stay_inside_the_extent(n, bw):
    """n = 9000 (71 block rows) is where the default chunk of 64 tiles splits block rows: the lists a handle uploads by
    default are executed here."""
    L, b, xref = reference(n, bw)
    extent = plan(n, bw)[1]
    d = np.arange(n)[:, None] - np.arange(n)[None, :]  # i - j
    W = L  # in place: NaN above the diagonal and beyond the extent
    W[(d < 0) | (d > extent)] = np.nan
    del d
    kb = band_lib().band_sweep_blocks_c(bw)
    for chunk in CHUNKS:
        y = run_sweep(W, b, n, kb, chunk, backward=False)
        x = run_sweep(W, y, n, kb, chunk, backward=True)
        assert not np.any(np.isnan(y)) and not np.any(np.isnan(x)), "nothing beyond the extent is read"
        assert np.linalg.norm(x - xref) / np.linalg.norm(xref) < 1e-10, (chunk, np.linalg.norm(x - xref) / np.linalg.norm(xref))


def test_sweep_plan_under_address_and_undefined_sanitizers():
    """tests/csrc_band/band_sweep_main.cpp: a stand-alone program (never loaded into Python) that walks the job
    lists of the shapes above the way the kernels read them."""
    band_lib()  # (runs make)
    out = subprocess.run([os.path.join(ROOT, "tests", "_build", "band_sweep_check")], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    assert "BAD" not in out.stdout and out.stdout.count(" ok") >= len(SHAPES) * len(CHUNKS)
