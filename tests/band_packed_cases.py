"""Helpers of the packed band storage tests (tests/test_band_packed.py, tests/test_gpu_band_packed.py): the layout of
madqp_jl_amd/csrc/band_plan.inc through its CPU build (tests/csrc_band_packed), packed buffers with NaN in every slot that
is no band entry, and the numpy view the plan is executed through."""
import ctypes as C
import os
import subprocess

import numpy as np

from band_cases import NB, ROOT

_lib = None
NAN_BITS = np.float64(np.nan).view(np.uint64)


def packed_lib():
    global _lib
    if _lib is None:
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "tests", "csrc_band_packed")], stdout=subprocess.DEVNULL)
        _lib = C.CDLL(os.path.join(ROOT, "tests", "_build", "libmadqp_band_packed.so"))
        i64 = C.c_int64
        _lib.band_packed_layout_c.restype = i64
        _lib.band_packed_layout_c.argtypes = [i64, i64, i64, i64, C.c_void_p]
        _lib.band_packed_default_pad_c.restype = i64
    return _lib


def layout(n, extent, ld_in=0, pad=-1):
    """(ld, doubles) of band_packed_layout, None where it refuses; ld_in <= 0: the library's choice"""
    out = (C.c_int64 * 2)()
    return (out[0], out[1]) if packed_lib().band_packed_layout_c(n, extent, ld_in, pad, out) else None


def npad(n):
    return (max(n, 1) + NB - 1) // NB * NB


def band_index(n, extent):
    """(i, j) of every entry with 0 <= i - j <= extent, column by column"""
    cnt = np.minimum(extent + 1, n - np.arange(n))  # entries of column j
    j = np.repeat(np.arange(n), cnt)
    i = np.arange(len(j)) - np.repeat(np.cumsum(cnt) - cnt, cnt) + j
    return i, j


def lds_to_test(n, extent):
    """the leading dimensions the issue asks for: the extent itself, extent + 1, the library's choice, extent + 37"""
    return [max(extent, 1), extent + 1, layout(n, extent)[0], extent + 37]


def pack(K, extent, ld, doubles):
    """A packed buffer of `doubles` doubles holding the entries 0 <= i - j <= extent of K at [i + j ld], NaN in every other
    slot (the gaps extent < i - j <= ld and the slack); returns (buffer, addresses of the band entries)."""
    n = K.shape[0]
    i, j = band_index(n, extent)
    addr = i + j * ld
    assert len(np.unique(addr)) == len(addr) and addr.max() < doubles
    buf = np.full(doubles, np.nan)
    buf[addr] = K[i, j]
    return buf, addr


def view(buf, n, ld):
    """the buffer as the column-major (npad, n) matrix the kernels address: [i, j] = buf[i + j ld].  Entries above the
    diagonal and beyond ld alias other columns -- what executes a plan through it must write neither."""
    assert (npad(n) - 1) + (n - 1) * ld < len(buf)
    return np.lib.stride_tricks.as_strided(buf, shape=(npad(n), n), strides=(8, 8 * ld))


def unpack(buf, n, extent, ld):
    """dense lower triangle from a packed buffer, zeros beyond the extent"""
    i, j = band_index(n, extent)
    L = np.zeros((n, n))
    L[i, j] = buf[i + j * ld]
    return L


def nan_kept(buf, addr):
    """every slot that is no band entry still holds the planted NaN, bit for bit"""
    mask = np.ones(len(buf), dtype=bool)
    mask[addr] = False
    return bool(np.all(buf.view(np.uint64)[mask] == NAN_BITS))
