"""CPU: the per-iteration trace of the batched engine at the C ABI (madqp_batch_set_trace / madqp_batch_trace) and the
argument handling of BatchedMPCSolver that needs no device.  tests/fake_backend.py has no batched engine (it carries the
single-problem drivers only), so everything past the constructor's own checks is in tests/test_gpu_batched_trace.py."""
import ctypes
import os
import re
import types

import pytest

import madqp_jl_amd as M
from madqp_jl_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MADQP_ERR_ARG = -1


def test_trace_symbols_are_exported_with_prototypes():
    lib = M.load_cdll()
    for name, args in (("madqp_batch_set_trace", [ctypes.c_void_p, ctypes.c_int64]),
                       ("madqp_batch_trace", [ctypes.c_void_p, ctypes.POINTER(ctypes.c_double),
                                              ctypes.POINTER(ctypes.c_int32)])):
        assert name in M.EXPORTED_SYMBOLS
        fn = getattr(lib, name)
        assert list(fn.argtypes) == args and fn.restype is ctypes.c_int32


def test_trace_record_layout_matches_header():
    hdr = open(os.path.join(ROOT, "include", "madqp.h")).read()
    assert int(re.search(r"#define MADQP_BATCH_TRACE_LEN (\d+)", hdr).group(1)) == len(_lib.BATCH_TRACE) == 10
    assert _lib.BATCH_TRACE == ("obj", "inf_pr", "inf_du", "inf_compl", "mu", "dnorm", "del_w", "alpha_p", "alpha_d",
                                "residual_ratio")
    order = re.search(r"MADQP_BATCH_TRACE_LEN doubles --([^-]*)--", hdr).group(1)
    assert tuple(w.strip(" *\n") for w in order.replace("\n", " ").split(",")) == _lib.BATCH_TRACE


def test_null_handle_is_an_argument_error_without_a_device():
    lib = M.load_cdll()
    assert lib.madqp_batch_set_trace(None, 4) == MADQP_ERR_ARG
    assert lib.madqp_batch_trace(None, None, None) == MADQP_ERR_ARG
    buf, cnt = (ctypes.c_double * 10)(), (ctypes.c_int32 * 1)()
    assert lib.madqp_batch_trace(None, buf, cnt) == MADQP_ERR_ARG


@pytest.mark.parametrize("trace", [0, -1, -300, 2.5, "yes", None])
def test_bad_trace_argument_raises_before_anything_else(trace):
    # (no backend, no problems worth the name: the check comes first)
    with pytest.raises(ValueError, match="trace"):
        M.BatchedMPCSolver([types.SimpleNamespace(nvar=1, ncon=0)], None, trace=trace)


def test_negative_refine_steps_raises():
    with pytest.raises(ValueError, match="refine_steps"):
        M.BatchedMPCSolver([types.SimpleNamespace(nvar=1, ncon=0)], None, refine_steps=-1)
