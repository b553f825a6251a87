"""Test problems with a sparse Hessian (test infrastructure; tests/test_sparse_hessian.py and
tests/test_gpu_sparse_hessian.py): the sparse-Jacobian family of ``oracle.qp.sparse_qp`` with a sparse, strictly
diagonally dominant H, and the patterns the assembly kernels are held to."""
import numpy as np

from oracle import qp as Q


def sparse_hessian(seed: int, n: int, p: int) -> np.ndarray:
    """Dense copy of a sparse SPD matrix.  From ``numpy.random.default_rng(seed)``, in row order i = 1 .. n-1: a Gaussian
    entry at (i, i-1), then Gaussian entries at ``rng.choice(i, size=min(p, i), replace=False)`` columns; the matrix is
    mirrored and the diagonal set to 1 + sum_j |h_ij|: strictly diagonally dominant, condition number ~ 10-15."""
    rng = np.random.default_rng(seed)
    H = np.zeros((n, n))
    for i in range(1, n):
        H[i, i - 1] = rng.standard_normal()
        k = min(p, i)
        vals = rng.standard_normal(k)  # (drawn before the columns: the order the recorded oracle runs below were made with)
        H[i, rng.choice(i, size=k, replace=False)] = vals
    H = H + H.T
    H[np.arange(n), np.arange(n)] = 1.0 + np.abs(H).sum(axis=1)
    return H


def sparse_hessian_qp(seed, n, m, per_row, p, equality_cons=()):
    """``oracle.qp.sparse_qp(seed, n, m, per_row, "lp", equality_cons=...)`` with ``H = sparse_hessian(seed, n, p)``."""
    qp = Q.sparse_qp(seed, n, m, per_row, "lp", equality_cons=equality_cons)
    qp.H = sparse_hessian(seed, n, p)
    qp.name = f"sparse-hessian-n{n}-m{m}-s{seed}"
    return qp


# (form, oracle kkt_system, seed, n, m, per_row, p, equality rows, oracle iterations): the whole-solve cases; the oracle
# ends SOLVE_SUCCEEDED after the same number of iterations with and without refine_steps=1 on every one of them, and the
# distance of those two runs stays below the stated per-iteration bar (parity.trace_tolerances)
CASES = (
    ("condensed", "condensed", 3, 200, 60, 10, 3, (), 11),
    ("condensed", "condensed", 3, 100, 40, 6, 3, (), 13),
    ("condensed", "condensed", 13, 257, 30, 4, 2, (), 13),
    ("augmented", "K2", 31, 160, 70, 4, 3, (2, 9, 33), 17),
    ("augmented", "K2", 11, 129, 40, 4, 1, (1,), 13),
)

PATTERNS = ("generator", "offdiag", "empty", "arrow", "zeros")


def pattern(name: str, n: int, seed: int = 5):
    """Lower-triangle entries ``(rows, cols, vals)`` of an n x n test Hessian:
    generator -- ``sparse_hessian(seed, n, 3)``;
    offdiag   -- its strict lower triangle times 0.02, NO stored diagonal entry (the diagonal of K is dvec alone);
    empty     -- no entry at all;
    arrow     -- first column and last row full (Gaussian / n), diagonal 3: row 0 of the symmetric pattern holds n entries
                 (n = 300: a second trip of a 256-thread loop) and every column has an entry in the last row;
    zeros     -- the generator's pattern, off-diagonal values times 0.02, with every third stored value an explicit 0.0
                 (diagonal entries among them)."""
    rng = np.random.default_rng(seed + 1000)
    if name == "empty":
        z = np.zeros(0, dtype=np.int64)
        return z, z, np.zeros(0)
    if name == "arrow":
        H = np.zeros((n, n))
        H[:, 0] = rng.standard_normal(n) / n
        H[n - 1, :] = rng.standard_normal(n) / n
        H[np.arange(n), np.arange(n)] = 3.0
        r, c = np.nonzero(np.tril(np.ones((n, n), dtype=bool) & ((np.arange(n)[None, :] == 0) | (np.arange(n)[:, None] == n - 1)
                                                                 | np.eye(n, dtype=bool))))
        return r, c, H[r, c]
    L = np.tril(sparse_hessian(seed, n, 3))
    if name == "offdiag":
        L = 0.02 * np.tril(L, -1)
    elif name == "zeros":  # (small off-diagonal entries: K stays positive definite where a zero sits on the diagonal)
        L = np.diag(np.diag(L)) + 0.02 * np.tril(L, -1)
    r, c = np.nonzero(L)
    v = L[r, c]
    if name == "zeros":
        v = v.copy()
        v[::3] = 0.0
    elif name not in ("generator", "offdiag"):
        raise ValueError(name)
    return r, c, v
