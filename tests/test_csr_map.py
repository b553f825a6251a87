"""CPU: COO -> CSR maps of the sparse front end (``madqp_csr_map_*``, include/madqp.h).

``madqp_csr_map_plan_host`` -- the one function ``madqp_csr_map_create`` builds from -- is held to numpy on the host: the
CSR structure is the sorted distinct destinations, the segments partition the sources, sources ascend within a segment,
and for the symmetric kind (i, j) and (j, i) list the same sources.  ``DeviceCSR.from_coo`` / ``DeviceSymCSR.from_coo``
(built on the same plan) equal the constructors fed with the merged matrix.  julia/MadQPHIPSparse.jl is checked
statically, as tests/test_abi.py checks julia/MadQPHIP.jl.  The device pass is tests/test_gpu_csr_map.py."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import julia_replay as JR
import madqp_jl_amd as M
from madqp_jl_amd import qp as QP

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KINDS = ("rows", "cols", "sym")
ERR_ARG = -1


def plan(I0, J0, nrows, ncols, kind, arrays=True):
    """``madqp_csr_map_plan_host`` on a 0-based pattern (handed over 1-based int32, as MadNLP's).  Returns the status and
    (sizes, ptr, col, seg, src); ``arrays=False``: the size-only call."""
    lib = M.load_cdll()
    I1 = np.ascontiguousarray(np.asarray(I0, dtype=np.int64) + 1, dtype=np.int32)
    J1 = np.ascontiguousarray(np.asarray(J0, dtype=np.int64) + 1, dtype=np.int32)
    sizes = (C.c_int64 * 3)(-7, -7, -7)
    k = kind if isinstance(kind, int) else KINDS.index(kind)
    head = (len(I1), I1.ctypes.data, J1.ctypes.data, nrows, ncols, k, sizes)
    rc = lib.madqp_csr_map_plan_host(*head, None, None, None, None)
    if rc != 0 or not arrays:
        return rc, (list(sizes),)
    rows, stored, sources = sizes
    # one spare slot behind every array, which the call must leave alone
    out = [np.full(k + 1, -99, dtype=np.int64) for k in (rows + 1, stored, stored + 1, sources)]
    sizes2 = (C.c_int64 * 3)()
    rc = lib.madqp_csr_map_plan_host(*head[:-1], sizes2, *[a.ctypes.data for a in out])
    assert list(sizes2) == list(sizes), "the size-only call and the full call disagree"
    assert all(a[-1] == -99 for a in out), "written past the stated sizes"
    return rc, (list(sizes),) + tuple(a[:-1] for a in out)


def expected(I0, J0, nrows, ncols, kind):
    """numpy: destination (row, column) -> its sources in ascending COO position."""
    dest = {}
    for k, (i, j) in enumerate(zip(I0, J0)):
        i, j = int(i), int(j)
        for d in {"rows": [(i, j)], "cols": [(j, i)], "sym": [(i, j)] + ([(j, i)] if i != j else [])}[kind]:
            dest.setdefault(d, []).append(k)
    keys = sorted(dest)
    rows = ncols if kind == "cols" else nrows
    ptr = np.concatenate([[0], np.cumsum(np.bincount(np.array([r for r, _ in keys], dtype=np.int64), minlength=rows))])
    return rows, ptr, np.array([c for _, c in keys], dtype=np.int64), [dest[k] for k in keys], keys


def check_plan(I0, J0, nrows, ncols, kind, what):
    rc, (sizes, ptr, col, seg, src) = plan(I0, J0, nrows, ncols, kind)
    assert rc == 0, what
    rows, e_ptr, e_col, e_src, keys = expected(I0, J0, nrows, ncols, kind)
    assert sizes == [rows, len(keys), sum(len(s) for s in e_src)], what
    assert np.array_equal(ptr, e_ptr) and np.array_equal(col, e_col), what  # the sorted distinct keys
    assert seg[0] == 0 and seg[-1] == len(src) and np.all(np.diff(seg) >= 1), what  # seg partitions src; none is empty
    for d in range(len(keys)):
        s = src[seg[d]:seg[d + 1]]
        assert np.all(np.diff(s) > 0), (what, keys[d])  # sources within a segment ascend
        assert list(s) == e_src[d], (what, keys[d])
    for r in range(rows):  # column indices strictly ascending within a row
        assert np.all(np.diff(col[ptr[r]:ptr[r + 1]]) > 0), (what, r)
    if kind == "sym":
        where = {k: d for d, k in enumerate(keys)}
        for (i, j), d in where.items():
            t = where[(j, i)]
            assert list(src[seg[d]:seg[d + 1]]) == list(src[seg[t]:seg[t + 1]]), (what, i, j)
    rc, (only,) = plan(I0, J0, nrows, ncols, kind, arrays=False)
    assert rc == 0 and only == sizes, what
    return sizes


def patterns():
    """(name, nrows, ncols, I, J), 0-based."""
    rng = np.random.default_rng(20251019)
    z = np.zeros(0, dtype=np.int64)
    out = [("nnz=0 with 5 rows", 5, 7, z, z), ("0 x 0", 0, 0, z, z), ("1 x 1 given three times", 1, 1, [0, 0, 0], [0, 0, 0]),
           ("1 x 9", 1, 9, np.zeros(9, dtype=np.int64), rng.permutation(9)),
           ("9 x 1", 9, 1, rng.permutation(9), np.zeros(9, dtype=np.int64))]
    i = np.array([1, 2, 4, 4, 1, 2, 2], dtype=np.int64)  # rows 0, 3 and 5 of 6 stay empty
    out.append(("first, middle and last row empty", 6, 5, i, np.array([0, 4, 2, 0, 3, 4, 1], dtype=np.int64)))
    j = np.concatenate([rng.permutation(8), [3, 3, 7]])
    out.append(("one row holding every entry", 5, 8, np.full(len(j), 2, dtype=np.int64), j))
    out.append(("one destination holding all 300 entries", 4, 4, np.full(300, 2, dtype=np.int64), np.full(300, 1, dtype=np.int64)))
    dense = rng.standard_normal((23, 58)) * (rng.random((23, 58)) < 0.3)
    I, J, _ = JR.coo_pattern(dense, rng, duplicates=9)
    out.append(("23 x 58 at density 0.3, shuffled, 9 duplicates", 23, 58, I.astype(np.int64) - 1, J.astype(np.int64) - 1))
    return out


def sym_patterns():
    rng = np.random.default_rng(37)
    n = 37
    G = rng.standard_normal((n, n)) * (rng.random((n, n)) < 0.25)
    out = []
    for name, A in (("tril", np.tril(G)), ("triu", np.triu(G)), ("diagonal only", np.diag(rng.standard_normal(n)))):
        I, J, _ = JR.coo_pattern(A, rng, duplicates=9)
        out.append((name, n, n, I.astype(np.int64) - 1, J.astype(np.int64) - 1))
    I, J, _ = JR.coo_pattern(np.tril(G), rng, duplicates=9)
    I, J = I.astype(np.int64) - 1, J.astype(np.int64) - 1
    flip = rng.random(len(I)) < 0.5  # half of the entries given in the other triangle ...
    I2, J2 = np.where(flip, J, I), np.where(flip, I, J)
    off = np.flatnonzero(I != J)[:11]  # ... and eleven pairs present as (i, j) AND (j, i)
    I2, J2 = np.concatenate([I2, J2[off]]), np.concatenate([J2, I2[off]])
    order = rng.permutation(len(I2))
    out.append(("mixed triangles, (i, j) and (j, i) both present", n, n, I2[order], J2[order]))
    return out


@pytest.mark.parametrize("kind", KINDS)
def test_plan_matches_numpy(kind):
    for name, nrows, ncols, I, J in patterns():
        if kind == "sym":  # (needs a square: the pattern sits in the leading corner of one)
            nrows = ncols = max(nrows, ncols)
        check_plan(I, J, nrows, ncols, kind, (kind, name))


def test_plan_symmetric_from_either_triangle():
    for name, n, _, I, J in sym_patterns():
        sizes = check_plan(I, J, n, n, "sym", name)
        if name == "diagonal only":
            assert sizes[1] == n and sizes[2] == len(I)  # a diagonal entry is stored, and fed, once
    # the same pairs from the lower and from the upper triangle of the same matrix: the same full pattern
    lo = [p for p in sym_patterns() if p[0] == "tril"][0]
    _, (s1, ptr1, col1, _, _) = plan(lo[3], lo[4], 37, 37, "sym")
    _, (s2, ptr2, col2, _, _) = plan(lo[4], lo[3], 37, 37, "sym")
    assert s1 == s2 and np.array_equal(ptr1, ptr2) and np.array_equal(col1, col2)


def test_plan_refusals_are_return_codes():
    ok = lambda: plan([0, 2], [1, 3], 3, 4, "rows")[0] == 0  # the process lives on and the next call is served
    assert ok()
    for kind in ("rows", "cols"):
        assert plan([0, -1], [1, 1], 3, 4, kind)[0] == ERR_ARG and ok()  # a (1-based) index 0
        assert plan([0, 3], [1, 1], 3, 4, kind)[0] == ERR_ARG and ok()  # a (1-based) row index nrows + 1
        assert plan([0, 1], [1, 4], 3, 4, kind)[0] == ERR_ARG and ok()  # a column index ncols + 1
        assert plan([], [], -1, 4, kind)[0] == ERR_ARG and plan([], [], 3, -1, kind)[0] == ERR_ARG and ok()
    assert plan([0], [1], 3, 4, "sym")[0] == ERR_ARG and ok()  # SYM on 3 x 4
    assert plan([0, -1], [1, 1], 4, 4, "sym")[0] == ERR_ARG and plan([0, 4], [1, 1], 4, 4, "sym")[0] == ERR_ARG and ok()
    assert plan([0], [1], 3, 4, 3)[0] == ERR_ARG and plan([0], [1], 3, 4, -1)[0] == ERR_ARG and ok()  # kind 3
    lib = M.load_cdll()
    one = np.ones(1, dtype=np.int32)
    sizes, buf = (C.c_int64 * 3)(), np.zeros(4, dtype=np.int64)
    assert lib.madqp_csr_map_plan_host(1, one.ctypes.data, one.ctypes.data, 2, 2, 0, None, None, None, None, None) == ERR_ARG
    assert lib.madqp_csr_map_plan_host(1, None, None, 2, 2, 0, sizes, None, None, None, None) == ERR_ARG  # no pattern
    assert lib.madqp_csr_map_plan_host(1, one.ctypes.data, one.ctypes.data, 2, 2, 0, sizes, buf.ctypes.data, None, None,
                                       None) == ERR_ARG  # some, not all, of the four arrays
    assert lib.madqp_csr_map_create(None, 0, None, None, 1, 1, 0, None) == ERR_ARG
    assert lib.madqp_csr_map_pattern(None, None, None, None, None) == ERR_ARG
    assert lib.madqp_csr_map_apply(None, None, None) == ERR_ARG
    assert lib.madqp_csr_map_destroy(None) == 0 and ok()


def merged(I, J, v, shape, symmetric=False):
    """The matrix a COO triple stands for, duplicates added in COO order from +0.0 (``numpy.add.at`` is unbuffered)."""
    I, J = np.asarray(I), np.asarray(J)
    if symmetric:  # every entry of the pair {i, j} counts for the lower-triangle position
        I, J = np.maximum(I, J), np.minimum(I, J)
    D, hit = np.zeros(shape), np.zeros(shape, dtype=bool)
    np.add.at(D, (I, J), v)
    hit[I, J] = True
    return D, hit


def test_from_coo_equals_the_constructor_fed_with_the_merged_matrix():
    rng = np.random.default_rng(8)
    for name, m, n, I, J in patterns():
        I, J = np.asarray(I, dtype=np.int64), np.asarray(J, dtype=np.int64)
        v = rng.standard_normal(len(I))
        got = M.DeviceCSR.from_coo("cpu", m, n, I, J, v)
        D, hit = merged(I, J, v, (m, n))
        r, c = np.nonzero(hit)
        want = M.DeviceCSR("cpu", m, n, r, c, D[r, c])
        for k in ("ptr", "col", "val", "t_ptr", "t_col", "t_perm", "row", "t_val"):
            assert torch.equal(getattr(got, k), getattr(want, k)), (name, k)
        assert (got.m, got.n, got.nnz) == (want.m, want.n, want.nnz) and got.ptr.dtype == torch.int64, name
        if len(set(zip(I.tolist(), J.tolist()))) < len(I):
            with pytest.raises(ValueError, match="duplicate entries"):  # the constructors keep refusing duplicates
                M.DeviceCSR("cpu", m, n, I, J, v)
    for name, n, _, I, J in sym_patterns():
        v = rng.standard_normal(len(I))
        got = M.DeviceSymCSR.from_coo("cpu", n, I, J, v)
        D, hit = merged(I, J, v, (n, n), symmetric=True)
        r, c = np.nonzero(hit)
        want = M.DeviceSymCSR("cpu", n, r, c, D[r, c])
        for k in ("ptr", "col", "val", "row"):
            assert torch.equal(getattr(got, k), getattr(want, k)), (name, k)
        assert (got.n, got.nnz, got.nnz_lower) == (want.n, want.nnz, want.nnz_lower), name
        assert torch.equal(got.to_dense(), got.to_dense().T), name  # the two triangles hold the same bits
        lo = np.maximum(I, J), np.minimum(I, J)
        with pytest.raises(ValueError, match="duplicate entries"):
            M.DeviceSymCSR("cpu", n, lo[0], lo[1], v)
    with pytest.raises(ValueError, match="above the diagonal"):
        M.DeviceSymCSR("cpu", 3, [0], [2], [1.0])
    with pytest.raises(ValueError):
        M.DeviceCSR.from_coo("cpu", 3, 4, [3], [0], [1.0])  # outside the matrix
    with pytest.raises(ValueError):
        M.DeviceSymCSR.from_coo("cpu", 3, [0], [-1], [1.0])
    assert QP.csr_plan([], [], 5, 7, "cols")[0] == 7


def test_julia_sparse_glue_binds_only_exported_symbols_and_defines_the_plugin_surface():
    """julia/MadQPHIPSparse.jl cannot run here (no Julia): every ccall target must exist in the library, and every
    method the reference calls on the KKT system must be defined for the sparse types (the GPU replay is
    tests/test_gpu_julia_sparse.py)."""
    src = open(os.path.join(ROOT, "julia", "MadQPHIPSparse.jl")).read()
    code = "\n".join(line.split("#", 1)[0] for line in src.splitlines())
    bound = set(re.findall(r"(?::|@k )(madqp_[a-z0-9_]+)", code))
    assert bound <= set(M.EXPORTED_SYMBOLS), sorted(bound - set(M.EXPORTED_SYMBOLS))
    assert {"madqp_csr_map_create", "madqp_csr_map_pattern", "madqp_csr_map_apply", "madqp_csr_map_destroy",
            "madqp_kkt_create_sparse", "madqp_kkt_set_hcsr", "madqp_kkt_set_refine"} <= bound
    assert not bound & {"madqp_coo_map_create", "madqp_coo_map_apply", "madqp_kkt_create", "madqp_kkt_create_augmented",
                        "madqp_kkt_create_normal"}  # no dense operand
    for method in ("MadNLP.create_kkt_system", "MadNLP.num_variables(kkt::HIPSparseKKTSystem",
                   "MadNLP.get_jacobian(kkt::HIPSparseKKTSystem", "MadNLP.get_hessian(kkt::HIPSparseKKTSystem",
                   "MadNLP.is_inertia_correct(kkt::HIPSparseKKTSystem", "MadNLP.initialize!(kkt::HIPSparseKKTSystem",
                   "MadNLP.compress_jacobian!(kkt::HIPSparseKKTSystem", "MadNLP.compress_hessian!(kkt::HIPSparseKKTSystem",
                   "MadNLP.jtprod!(y::AbstractVector, kkt::HIPSparseKKTSystem", "MadNLP.build_kkt!(kkt::HIPSparseKKTSystem",
                   "MadNLP.solve!(kkt::HIPSparseKKTSystem", "mul!(w::MadNLP.AbstractKKTVector{T}, kkt::HIPSparseKKTSystem",
                   "MadIPM.set_aug_diagonal_reg!(kkt::HIPSparseKKTSystem", "MadIPM.set_initial_primal_rhs!",
                   "MadIPM.set_initial_dual_rhs!", "MadIPM.set_predictive_rhs!", "MadIPM.set_correction_rhs!",
                   "MadIPM.get_correction!", "MadIPM.set_extra_correction!", "MadIPM.get_complementarity_measure",
                   "MadIPM.get_affine_complementarity_measure", "MadIPM.get_fraction_to_boundary_step",
                   "HIPSparseCondensedKKTSystem", "HIPSparseAugmentedKKTSystem", "HIPSparseNormalKKTSystem",
                   "The KKT system NormalKKTSystem supports only linear programs."):
        assert method in src, method
    # what it borrows from the dense glue exists there under that name
    dense = open(os.path.join(ROOT, "julia", "MadQPHIP.jl")).read()
    imported = re.search(r"import \.\.MadQPHIP: (.*)", src).group(1).replace("@", "").split(", ")
    for name in imported:
        assert re.search(r"(struct|const|macro|function)? ?\b%s\b" % name, dense), name
    # the kind constants follow the header's enum
    hdr = open(os.path.join(ROOT, "include", "madqp.h")).read()
    enum = re.search(r"enum \{ MADQP_CSR_ROWS = (\d), MADQP_CSR_COLS = (\d), MADQP_CSR_SYM = (\d) \};", hdr).groups()
    assert enum == ("0", "1", "2") == tuple(re.search(r"const CSR_%s = Int32\((\d)\)" % k, src).group(1)
                                            for k in ("ROWS", "COLS", "SYM"))
    assert M._lib.CSR_KINDS == KINDS
