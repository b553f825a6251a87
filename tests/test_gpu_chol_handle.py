"""GPU: the lifetimes of one Cholesky handle that replace its buffers -- the band's job list across several
``madqp_chol_set_bandwidth`` calls beside the dense sweeps' own list, and the workspace of ``madqp_chol_solve_many`` across
block sizes.  After every step the handle computes, bit for bit, what a fresh handle computes that was given that one
configuration only: no tolerance is involved."""
import numpy as np
import pytest

import madqp_jl_amd as M
from band_cases import workgroups
from test_gpu_band import bits, dev, leading_dimension, reference
from test_gpu_band_sweeps import create

pytestmark = pytest.mark.gpu

ERR_STATE = -4


def stored(n, bw, lda):
    """the reference matrix of half-bandwidth bw, column-major with leading dimension lda, zeros outside the band"""
    K, _ = reference(n, bw)
    host = np.zeros((n, lda))
    host[:, :n] = K.T
    return host


def factor_and_solve_two(hip, h, host, lda, n):
    """the factor and the solutions of two right-hand sides, one madqp_chol_solve each"""
    rng = np.random.default_rng(n + lda)
    Kd = dev(host, hip)
    assert hip.chol_factor(h, Kd, lda) == 0
    xs = []
    for _ in range(2):
        bd = dev(rng.standard_normal(n), hip)
        hip.chol_solve(h, bd)
        xs.append(bd.cpu().numpy())
    assert not np.any(np.isnan(xs[0])) and not np.any(np.isnan(xs[1]))
    return Kd.cpu().numpy(), xs[0], xs[1]


def test_one_handle_across_bandwidths_with_job_lists(hip):
    """n = 1537 under MADQP_SWEEP_CHUNK=2: 13 block rows against chunks of 2 tiles, so the dense sweeps have a job list and the
    band sweeps one of their own, which every madqp_chol_set_bandwidth replaces or frees."""
    n, chunk = 1537, 2
    nblk = (n + 127) // 128
    lda = leading_dimension(n, True)
    h = create(hip, n, MADQP_SWEEP_CHUNK=chunk)
    try:
        for bw in (None, 300, 127, -1, 300):  # None: the handle as created
            fresh = create(hip, n, MADQP_SWEEP_CHUNK=chunk)
            try:
                if bw is not None:
                    hip.chol_set_bandwidth(h, bw)
                banded = bw is not None and bw >= 0
                if banded:
                    hip.chol_set_bandwidth(fresh, bw)
                kb = (bw + 127) // 128 if banded else -1
                info = hip.chol_sweep_info(h)
                assert info == hip.chol_sweep_info(fresh) == (kb, workgroups(n, kb, chunk), chunk)
                assert workgroups(n, -1, chunk) > nblk and workgroups(n, 3, chunk) > nblk, "both forms have a job list"
                assert hip.chol_band_extent(h) == hip.chol_band_extent(fresh)
                if bw == -1:  # what is stored was factored under the band: no solve before the next factorisation
                    b = np.random.default_rng(7).standard_normal(n)
                    bd = dev(b, hip)
                    assert hip.lib.madqp_chol_solve(h, M._lib.ptr(bd)) == ERR_STATE
                    assert np.array_equal(bits(bd.cpu().numpy()), bits(b)), "a refused solve leaves the right-hand side alone"
                host = stored(n, bw if banded else n - 1, lda)
                got, ref = (factor_and_solve_two(hip, k, host, lda, n) for k in (h, fresh))
                for a, b, what in zip(got, ref, ("factor", "first solution", "second solution")):
                    assert np.array_equal(bits(a), bits(b)), f"bw={bw}: the {what}"
            finally:
                hip.chol_destroy(fresh)
    finally:
        hip.chol_destroy(h)


@pytest.mark.parametrize("padded", [True, False], ids=["padded-with-U", "unpadded"])
def test_one_handle_across_block_sizes(hip, padded):
    """n = 300 (padded: a mid-size factor with U = L'; unpadded: left-looking, the strip of L' in the workspace): blocks of
    32, 96 and 32 right-hand sides -- the transposed block has a leading dimension of whole 128s, so the workspace grows once,
    at the first call, and is used again -- then 160 and 32: it is replaced by a larger one and never shrinks."""
    n = 300
    lda = leading_dimension(n, padded)
    host = stored(n, n - 1, lda)
    rng = np.random.default_rng(n + lda)

    def factored():
        k = hip.chol_create(n)
        hip.chol_set_solve_many_min(k, 2)
        Kd = dev(host, hip)
        assert hip.chol_factor(k, Kd, lda) == 0
        return k, Kd

    h, Kh = factored()
    try:
        assert hip.chol_solve_many_info(h, 32)[2] == 0, "no workspace before the first blocked solve"
        sizes = []
        for nrhs in (32, 96, 32, 160, 32):
            B = rng.standard_normal((nrhs, n + 4))
            fresh, Kf = factored()
            try:
                out = []
                for k in (h, fresh):
                    Bd = dev(B, hip)
                    hip.chol_solve_many(k, Bd)
                    out.append(Bd.cpu().numpy())
                    assert hip.chol_solve_many_info(k, nrhs)[0] == 1, "the blocked path"
                assert not np.any(np.isnan(out[1][:, :n]))
                assert np.array_equal(bits(out[0]), bits(out[1])), f"the block of {nrhs} right-hand sides"
                sizes.append((hip.chol_solve_many_info(h, nrhs)[2], hip.chol_solve_many_info(fresh, nrhs)[2]))
            finally:
                hip.chol_destroy(fresh)
        npad = (n + 127) // 128 * 128
        small, large = (128 * npad + (0 if padded else 128 * npad), 256 * npad + (0 if padded else 128 * npad))  # solve_plan.inc
        assert [f for _, f in sizes] == [small, small, small, large, small], "a fresh handle's workspace is the block's own"
        assert [w for w, _ in sizes] == [small, small, small, large, large], "grown at the first call and for 160 columns, never shrunk"
    finally:
        hip.chol_destroy(h)
