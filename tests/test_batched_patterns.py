"""CPU: the host side of per-problem patterns in the batched engine -- ``pack_patterns`` builds, problem by problem, the
index lists ``get_index_constraints`` builds (CSR form), and the padded gather of the slack rows; the new C entry point
refuses a null context with a return code."""
import numpy as np
import pytest

import madqp_jl_amd as M
from madqp_jl_amd.batched import pack_patterns
from madqp_jl_amd.solver import get_index_constraints


def random_patterns(rng, B, nx, m):
    lvar, uvar = np.zeros((B, nx)), np.ones((B, nx))
    lcon, ucon = np.zeros((B, m)), np.ones((B, m))
    for b in range(B):
        kind = b % 5
        if kind == 0:  # no bounds, every row an equality: nlb = nub = 0, ns_b = 0
            lvar[b], uvar[b] = -np.inf, np.inf
            ucon[b] = lcon[b] = 0.25
        elif kind == 1:  # boxes and two-sided rows everywhere: ns_b = m
            pass
        else:  # a random mix of free / lower-only / upper-only / boxed variables, equality / one-sided / ranged rows
            v = rng.integers(0, 4, nx)
            lvar[b, v == 0], uvar[b, v == 0] = -np.inf, np.inf
            uvar[b, v == 1] = np.inf
            lvar[b, v == 2] = -np.inf
            r = rng.integers(0, 4, m)
            lcon[b, r == 0] = ucon[b, r == 0] = 0.1
            ucon[b, r == 1] = np.inf
            lcon[b, r == 2] = -np.inf
    return lvar, uvar, lcon, ucon


@pytest.mark.parametrize("B,nx,m,seed", [(11, 7, 5, 0), (5, 1, 1, 1), (6, 9, 0, 2), (8, 30, 12, 3)])
def test_pack_patterns_matches_get_index_constraints(B, nx, m, seed):
    rng = np.random.default_rng(seed)
    lvar, uvar, lcon, ucon = random_patterns(rng, B, nx, m)
    p = pack_patterns(lvar, uvar, lcon, ucon, "relax_bound")
    for key in ("ineq_ptr", "lb_ptr", "ub_ptr"):
        assert p[key].dtype == np.int64 and p[key].shape == (B + 1,) and p[key][0] == 0
        assert np.all(np.diff(p[key]) >= 0)
    ns = [len(get_index_constraints(lvar[b], uvar[b], lcon[b], ucon[b], "relax_bound")["ind_ineq"]) for b in range(B)]
    assert p["ns_max"] == max(ns) and list(p["ns"]) == ns
    assert p["gather"].shape == p["mask"].shape == (B, max(ns))
    for b in range(B):
        ic = get_index_constraints(lvar[b], uvar[b], lcon[b], ucon[b], "relax_bound")
        for key, ptr in (("ind_ineq", "ineq_ptr"), ("ind_lb", "lb_ptr"), ("ind_ub", "ub_ptr")):
            got = p[key][p[ptr][b]:p[ptr][b + 1]]
            assert got.dtype == np.int64 and np.array_equal(got, ic[key]), (b, key)
        k = len(ic["ind_ineq"])
        assert np.array_equal(p["mask"][b], np.arange(max(ns)) < k)
        assert np.array_equal(p["gather"][b, :k], ic["ind_ineq"]) and np.all(p["gather"][b, k:] == 0)
    assert p["any_eq"] == any(n < m for n in ns)
    if m:  # the generator covers the edges: ns_b = 0, ns_b = m, empty bound lists
        assert 0 in ns and m in ns
        assert np.any(np.diff(p["lb_ptr"]) == 0) and np.any(np.diff(p["ub_ptr"]) == 0)


def test_pack_patterns_fixed_variables_follow_the_treatment():
    lvar, uvar = np.array([[0.0, 1.0], [0.0, 0.0]]), np.array([[1.0, 1.0], [1.0, 2.0]])
    lcon = ucon = np.zeros((2, 0))
    p = pack_patterns(lvar, uvar, lcon, ucon, "relax_bound")
    assert list(p["lb_ptr"]) == [0, 2, 4] and list(p["ub_ptr"]) == [0, 2, 4] and p["ns_max"] == 0
    with pytest.raises(NotImplementedError):
        pack_patterns(lvar, uvar, lcon, ucon, "error")


def test_create_patterns_without_context_is_an_error_code():
    lib = M.load_cdll()
    assert lib.madqp_batch_create_patterns(None, 1, 1, 0, None, None, None, None, None, None, None, None, None) == -1
