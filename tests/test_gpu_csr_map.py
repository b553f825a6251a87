"""GPU: ``madqp_csr_map_apply`` (csrc/coo.hip) -- callback values in COO order -> the stored values of a CSR operand.

Bits: every stored value equals the sequential float64 sum of its sources from +0.0 in COO order (``numpy.add.at`` on
zeros, which is unbuffered and takes the indices in order); the output buffer holds NaN before the call, so an entry that
is not written shows.  Agreement: the CSR scattered into zeros has the bits of the dense operand ``madqp_coo_map_apply``
writes for the same pattern and values.  The structure itself is held to numpy in tests/test_csr_map.py (no GPU)."""
import numpy as np
import pytest
import torch

import julia_replay as JR
import madqp_jl_amd as M

pytestmark = pytest.mark.gpu
KINDS = ("rows", "cols", "sym")
GUARD = 64  # doubles behind the output that the pass must leave alone


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def destinations(I, J, nrows, ncols, kind):
    """numpy, independent of the library: (sorted distinct keys, per COO position its destination(s) in key order --
    an (nnz, 2) array, -1 where an entry has no second destination)."""
    I, J = np.asarray(I, dtype=np.int64), np.asarray(J, dtype=np.int64)
    width = nrows if kind == "cols" else ncols
    k1 = (J * width + I) if kind == "cols" else (I * width + J)
    k2 = np.where(I != J, J * width + I, -1) if kind == "sym" else np.full(len(I), -1, dtype=np.int64)
    keys = np.unique(np.concatenate([k1, k2[k2 >= 0]]))
    d = np.stack([np.searchsorted(keys, k1), np.where(k2 >= 0, np.searchsorted(keys, np.maximum(k2, 0)), -1)], axis=1)
    return keys, d, width


def reference(I, J, vals, nrows, ncols, kind):
    keys, d, width = destinations(I, J, nrows, ncols, kind)
    flat, v = d.ravel(), np.repeat(np.asarray(vals, dtype=np.float64), 2)  # COO order, an entry's two destinations side by side
    out = np.zeros(len(keys))
    np.add.at(out, flat[flat >= 0], v[flat >= 0])
    rows = ncols if kind == "cols" else nrows
    ptr = np.concatenate([[0], np.cumsum(np.bincount(keys // max(width, 1), minlength=rows))]) if rows else np.zeros(1, dtype=np.int64)
    return ptr, keys % max(width, 1), out


def run_map(hip, I, J, vals, nrows, ncols, kind):
    """create -> pattern -> apply into a NaN-filled buffer; returns (ptr, col, stored values), all on the host."""
    mp = M.CSRMap(hip, np.asarray(I, dtype=np.int64) + 1, np.asarray(J, dtype=np.int64) + 1, nrows, ncols, kind)
    try:
        ptr, col = mp.pattern_host()
        buf = torch.full((mp.stored + GUARD,), float("nan"), dtype=torch.float64, device=hip.device)
        buf[mp.stored:] = 7.0
        v = torch.as_tensor(np.asarray(vals, dtype=np.float64), device=hip.device)
        mp.apply(v if len(vals) else None, buf[: mp.stored] if mp.stored else buf[:0])
        host = buf.cpu().numpy()
        assert np.all(host[mp.stored:] == 7.0), "written past the stored entries"
        assert mp.rows == len(ptr) - 1 and mp.stored == len(col) == ptr[-1]
        return ptr, col, host[: mp.stored]
    finally:
        mp.close()


def check_bits(hip, I, J, vals, nrows, ncols, kind, what):
    ptr, col, out = run_map(hip, I, J, vals, nrows, ncols, kind)
    e_ptr, e_col, e_out = reference(I, J, vals, nrows, ncols, kind)
    assert np.array_equal(ptr, e_ptr) and np.array_equal(col, e_col), what
    assert np.array_equal(bits(out), bits(e_out)), (what, int(np.count_nonzero(bits(out) != bits(e_out))))
    return ptr, col, out


def pattern_with_stored(rng, n, stored, dups):
    """`stored` distinct positions of an n x n matrix in shuffled order, `dups` of them given a second and third time."""
    pos = rng.choice(n * n, size=stored, replace=False)
    pos = np.concatenate([pos, rng.choice(pos, size=dups, replace=False), rng.choice(pos, size=dups, replace=False)])
    pos = pos[rng.permutation(len(pos))]
    return pos // n, pos % n


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("stored", [255, 256, 257])
def test_bits_around_one_workgroup(hip, kind, stored):
    """255, 256 and 257 stored entries: one workgroup short of, exactly, and one past its 256 lanes.  (For the symmetric
    kind the count is set by diagonal entries plus mirrored pairs: 255 = 5 + 2 * 125, 256 = 2 * 128, 257 = 1 + 2 * 128.)"""
    rng = np.random.default_rng(stored)
    n = 41
    if kind == "sym":
        ndiag, npair = {255: (5, 125), 256: (0, 128), 257: (1, 128)}[stored]
        li, lj = np.tril_indices(n, -1)
        pick = rng.choice(len(li), size=npair, replace=False)
        dg = rng.choice(n, size=ndiag, replace=False)
        I, J = np.concatenate([li[pick], dg]), np.concatenate([lj[pick], dg])
        flip = rng.random(len(I)) < 0.3  # some in the upper triangle
        I, J = np.where(flip, J, I), np.where(flip, I, J)
        extra = rng.choice(len(I), size=9, replace=False)  # duplicates, given the other way round
        I, J = np.concatenate([I, J[extra]]), np.concatenate([J, I[extra]])
        order = rng.permutation(len(I))
        I, J = I[order], J[order]
    else:
        I, J = pattern_with_stored(rng, n, stored, 9)
    ptr, col, _ = check_bits(hip, I, J, rng.standard_normal(len(I)), n, n, kind, (kind, stored))
    assert len(col) == stored


@pytest.mark.parametrize("kind", KINDS)
def test_bits_edge_cases(hip, kind):
    rng = np.random.default_rng(3)
    # one destination of 300 sources (a serial sum by one lane), beside ordinary entries
    I = np.concatenate([np.full(300, 4), rng.integers(0, 9, 40)])
    J = np.concatenate([np.full(300, 2), rng.integers(0, 9, 40)])
    order = rng.permutation(len(I))
    check_bits(hip, I[order], J[order], rng.standard_normal(len(I)) * 10.0 ** rng.integers(-8, 8, len(I)), 9, 9, kind,
               (kind, "300 sources"))
    # NaN, +inf, -inf and a lone -0.0.  Each special value has a destination of its own, or shares one with finite values
    # only: the sum then PROPAGATES it (0.0 + -0.0 = +0.0, x + inf = inf, x + NaN = that quiet NaN), which every IEEE adder
    # does alike; inf - inf would CREATE a NaN, whose sign differs between host and device adders.
    I = np.array([0, 1, 2, 3, 5, 5, 6, 6, 7, 7, 8])
    J = np.array([0, 0, 1, 2, 4, 4, 0, 0, 3, 3, 8])
    v = np.array([np.nan, np.inf, -np.inf, -0.0, 1.5, np.nan, np.inf, 2.5, -1.0, -np.inf, 3.0])
    _, _, out = check_bits(hip, I, J, v, 9, 9, kind, (kind, "special values"))
    assert np.count_nonzero(np.isnan(out)) == (3 if kind == "sym" else 2)  # (0, 0) is diagonal; (5, 4) is mirrored for sym
    assert not np.any(np.signbit(out[out == 0.0]))  # the lone -0.0 comes out as +0.0: the sum starts from +0.0
    # nnz = 0: nothing stored, nothing launched; NULL buffers are fine
    z = np.zeros(0, dtype=np.int64)
    ptr, col, out = run_map(hip, z, z, np.zeros(0), 5, 5, kind)
    assert np.array_equal(ptr, np.zeros(6, dtype=np.int64)) and len(col) == len(out) == 0
    ptr, col, out = run_map(hip, z, z, np.zeros(0), 0, 0, kind)
    assert np.array_equal(ptr, np.zeros(1, dtype=np.int64)) and len(col) == 0


def test_bits_beyond_one_trip_of_the_grid_stride_loop(hip):
    """4096 workgroups of 256 lanes cover 1 048 576 destinations per trip: 1 100 000 distinct destinations on 2 000 x
    2 000 send 51 424 lanes round a second time.  (The cap is csrc/coo.hip's apply_grid.)"""
    rng = np.random.default_rng(11)
    n, stored = 2000, 1_100_000
    assert stored > 4096 * 256
    I, J = pattern_with_stored(rng, n, stored, 1000)
    _, col, _ = check_bits(hip, I, J, rng.standard_normal(len(I)), n, n, "rows", "1.1e6 destinations")
    assert len(col) == stored


def test_apply_refuses_null_buffers_before_any_launch(hip):
    mp = M.CSRMap(hip, [1, 2], [2, 1], 2, 2, "rows")
    out = torch.zeros(2, dtype=torch.float64, device=hip.device)
    v = torch.ones(2, dtype=torch.float64, device=hip.device)
    for a, b in ((None, out), (v, None)):
        with pytest.raises(M.MadQPError, match=r"error -1: bad argument"):
            hip.csr_map_apply(mp._h, a, b)
    mp.apply(v, out)  # the context stays usable
    assert out.tolist() == [1.0, 1.0]
    mp.close()
    with pytest.raises(M.MadQPError, match=r"outside 2 x 2"):
        M.CSRMap(hip, [1, 3], [2, 1], 2, 2, "rows")
    with pytest.raises(M.MadQPError):
        M.CSRMap(hip, [1], [2], 2, 3, "sym")


def dense_route(hip, I, J, vals, nrows, ncols, symmetric):
    """What ``madqp_coo_map_apply`` writes for the pattern: the dense operand of the dense glue."""
    I1, J1 = (np.asarray(I) + 1).astype(np.int32), (np.asarray(J) + 1).astype(np.int32)
    h = JR.C.c_void_p()
    hip._ck(hip.lib.madqp_coo_map_create(hip.ctx, len(I1), I1.ctypes.data, J1.ctypes.data, nrows, ncols, symmetric, JR.C.byref(h)))
    dst = torch.full((nrows, ncols), 7.0, dtype=torch.float64, device=hip.device)
    hip._ck(hip.lib.madqp_coo_map_apply(h, M._lib.ptr(torch.as_tensor(vals, device=hip.device)), M._lib.ptr(dst), ncols))
    out = dst.cpu().numpy()
    hip.lib.madqp_coo_map_destroy(h)
    return out


def scatter(ptr, col, val, ncols):
    D = np.zeros((len(ptr) - 1, ncols))
    D[np.repeat(np.arange(len(ptr) - 1), np.diff(ptr)), col] = val
    return D


def test_csr_expands_to_the_bits_of_the_dense_route(hip):
    rng = np.random.default_rng(5)
    dense = rng.standard_normal((23, 58)) * (rng.random((23, 58)) < 0.3)
    I, J, v = JR.coo_pattern(dense, rng, duplicates=9)
    I, J = I.astype(np.int64) - 1, J.astype(np.int64) - 1
    v = v * rng.uniform(0.5, 2.0, len(v))  # (so that duplicates do not add up exactly)
    ptr, col, val = run_map(hip, I, J, v, 23, 58, "rows")
    assert np.array_equal(bits(scatter(ptr, col, val, 58)), bits(dense_route(hip, I, J, v, 23, 58, 0)))
    # COLS = ROWS of the transposed pattern, structure and values
    t = run_map(hip, I, J, v, 23, 58, "cols")
    r = run_map(hip, J, I, v, 58, 23, "rows")
    assert all(np.array_equal(a, b) for a, b in zip(t[:2], r[:2])) and np.array_equal(bits(t[2]), bits(r[2]))
    assert np.array_equal(bits(scatter(*t, 23)), bits(scatter(ptr, col, val, 58).T))
    # SYM against symmetric = 1, from one triangle and from mixed triangles with (i, j) and (j, i) both present
    G = rng.standard_normal((37, 37)) * (rng.random((37, 37)) < 0.3)
    I, J, v = JR.coo_pattern(np.tril(G), rng, duplicates=9)
    I, J = I.astype(np.int64) - 1, J.astype(np.int64) - 1
    v = v * rng.uniform(0.5, 2.0, len(v))
    flip = rng.random(len(I)) < 0.5
    off = np.flatnonzero(I != J)[:11]
    Im, Jm = np.where(flip, J, I), np.where(flip, I, J)
    Im, Jm, vm = np.concatenate([Im, Jm[off]]), np.concatenate([Jm, Im[off]]), np.concatenate([v, rng.standard_normal(11)])
    for name, (a, b, w) in (("tril", (I, J, v)), ("triu", (J, I, v)), ("mixed", (Im, Jm, vm))):
        ptr, col, val = run_map(hip, a, b, w, 37, 37, "sym")
        S = scatter(ptr, col, val, 37)
        assert np.array_equal(bits(S), bits(S.T)), name  # the two stored values of a pair are bitwise equal
        assert np.array_equal(bits(S), bits(dense_route(hip, a, b, w, 37, 37, 1))), name
