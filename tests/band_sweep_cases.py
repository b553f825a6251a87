"""Helpers of the band sweep tests (tests/test_band_sweep_plan.py, tests/test_gpu_band_sweeps.py): the job lists of
madqp_jl_amd/csrc/band_plan.inc through their CPU build (tests/csrc_band_sweep), and what the kernels make of a job."""
import ctypes as C
import os
import subprocess

import numpy as np

from band_cases import ROOT

_lib = None


def sweep_lib():
    global _lib
    if _lib is None:
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "tests", "csrc_band_sweep")], stdout=subprocess.DEVNULL)
        _lib = C.CDLL(os.path.join(ROOT, "tests", "_build", "libmadqp_band_sweep.so"))
        i64 = C.c_int64
        for name, args in (("band_sweep_blocks_c", [i64]), ("band_sweep_reach_c", [i64, i64]),
                           ("band_sweep_jobs_c", [i64, i64, i64, C.c_void_p, i64, C.c_void_p]),
                           ("band_plan_extent_c", [i64, i64, i64])):
            getattr(_lib, name).restype = i64
            getattr(_lib, name).argtypes = args
    return _lib


def sweep_jobs(nblk, kb, chunk):
    """((r, c) per ticket, maxc) of one sweep; kb < 0: the dense list"""
    lib = sweep_lib()
    cap = nblk * (nblk + 1) // 2 + nblk + 1
    out = np.zeros(cap, dtype=np.int32)
    cnt = C.c_int64(0)
    maxc = lib.band_sweep_jobs_c(nblk, kb, chunk, out.ctypes.data, cap, C.byref(cnt))
    assert 0 < cnt.value <= cap
    return [(int(j) & 0xFFFFF, int(j) >> 20) for j in out[: cnt.value]], int(maxc)


def dense_jobs(nblk, chunk):
    """the list madqp_chol_create builds"""
    return [(r, c) for r in range(nblk) for c in range(max(1, (r + chunk - 1) // chunk))]


def ranges(r, c, kb, chunk):
    """what the kernels make of job (r, c): its tiles [j0, j1), whether it owns the row, the first chunk it waits for"""
    lo = max(0, r - kb) if kb >= 0 else 0
    j0, j1 = max(c * chunk, lo), min(r, (c + 1) * chunk)
    return j0, j1, j1 == r, lo // chunk


def workgroups(n, kb, chunk):
    """workgroups of one sweep of a handle of order n (madqp_chol_sweep_info): the job count where block rows are split"""
    nblk = max(1, (n + 127) // 128)
    return len(sweep_jobs(nblk, kb, chunk)[0]) if nblk - 1 > chunk else nblk
