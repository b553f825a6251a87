"""GPU: a sparse Hessian (``DeviceSymCSR``, ``madqp_kkt_set_hcsr``) in the sparse-Jacobian front end -- condensed and
augmented form.  The assembled matrix must have the BITS of the one the same front end assembles from the dense form of
the same H; ``mul!`` and ``eval`` are held to an extended-precision evaluation with the derived bound of DESIGN.md
section 3.1; whole solves to the CPU oracle; the ABI refuses what it does not serve with a return code."""
import functools

import numpy as np
import pytest
import torch

import madqp_jl_amd as M
import parity
from oracle import mpc
from oracle import qp as Q
from sparse_hessian import CASES, PATTERNS, pattern, sparse_hessian_qp

pytestmark = pytest.mark.gpu
REG = M.FixedRegularization(1e-8, -1e-8)
U = 2.0 ** -53
LD = np.longdouble
STATE_VECTORS = M.State.VEC_N + M.State.VEC_M + M.State.KKT + ("correction_lb", "l_diag", "l_lower", "correction_ub",
                                                                "u_diag", "u_lower")


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def device_qp(qp, be, H):
    dq = M.DeviceQP.from_numpy(be.device, None, qp.q, qp.A, qp.lvar, qp.uvar, qp.lcon, qp.ucon, qp.x0, qp.c0, sparse=True)
    dq.H = H
    return dq


def whole_matrix(be, kkt, order):
    """Every stored double of the first ``order`` columns of the library's K (ld x order, padding rows included)."""
    ptr, ld = be.kkt_matrix(kkt._h, order)
    return be.read_doubles(ptr, ld * order).reshape(order, ld).T  # [i, j] = K[i + j * ld]


def built_pair(be, nx, name, form, scaling):
    """The same problem through the sparse front end twice -- H as DeviceSymCSR and as its ``to_dense()`` -- initialised,
    with ONE state (the dense run's: the two start points differ in the rounding of H x, and K is compared bit for bit, so
    both objects must see the same Sigma), regularised and assembled, NOT factorised.  Returns (sparse-H solver, dense-H
    solver)."""
    m = max(1, nx // 3)
    qp = Q.sparse_qp(40 + nx, nx, m, 2, "lp")
    r, c, v = pattern(name, nx)
    hs = M.DeviceSymCSR(be.device, nx, r, c, v)
    assert hs.nnz_lower == len(v)
    kw = dict(kkt_system=form, scaling=scaling)
    if form == "condensed":
        kw["regularization"] = REG
    ss = M.MPCSolver(device_qp(qp, be, hs), be, **kw)
    sd = M.MPCSolver(device_qp(qp, be, hs.to_dense().contiguous()), be, **kw)
    for s in (ss, sd):
        s.initialize()
    assert isinstance(ss.H, M.DeviceSymCSR) and torch.is_tensor(sd.H) and sd.H.dim() == 2
    assert type(ss.kkt) is type(sd.kkt) and type(ss.kkt).__name__.startswith("HIPSparse")
    assert ss.obj_scale == sd.obj_scale and torch.equal(ss.A.val, sd.A.val)
    assert torch.equal(ss.H.to_dense(), sd.H)  # the scaled copies hold the same values
    for k in STATE_VECTORS:
        getattr(ss.st, k).copy_(getattr(sd.st, k))
    for s in (ss, sd):
        s.kkt.set_aug_diagonal_reg(1.0, -1e-8)
        s.kkt.build_kkt()
    return ss, sd


@pytest.mark.parametrize("form", ["condensed", "augmented"])
@pytest.mark.parametrize("nx", [1, 2, 127, 128, 129, 257, 300])
def test_assembly_has_the_bits_of_the_dense_hessian_path(hip, nx, form):
    m = max(1, nx // 3)
    order = nx if form == "condensed" else (nx + 127) // 128 * 128 + m
    for name in PATTERNS:
        for scaling in (True, False):
            ss, sd = built_pair(hip, nx, name, form, scaling)
            Ks, Kd = whole_matrix(hip, ss.kkt, order), whole_matrix(hip, sd.kkt, order)
            what = (form, nx, name, scaling)
            low = np.tril_indices(order)
            assert np.array_equal(bits(Ks[:order][low]), bits(Kd[:order][low])), what  # the lower triangle that is factorised
            assert np.array_equal(bits(Ks), bits(Kd)), what  # strict upper triangle, identity padding, rows past the order
            # ... and it is the matrix: H + Sigma_x (+ A' Theta A) resp. [H + Sigma_x, .; A, -D] on the host copies
            H, A = sd.H.cpu().numpy(), sd.A.to_dense().cpu().numpy()
            pr = sd.st.pr_diag.cpu().numpy()
            if form == "augmented":
                np_ = order - m
                assert np.array_equal(np.tril(Ks[:nx, :nx]), np.tril(H + np.diag(pr[:nx]))), what
                assert np.array_equal(Ks[np_:order, :nx], A) and np.array_equal(Ks[nx:np_, nx:np_], np.eye(np_ - nx)), what
            else:  # (the Gram term adds w V V' with positive weights: the diagonal can only grow over H + Sigma_x)
                assert np.all(np.isfinite(Ks[:order][low])) and np.all(np.diag(Ks[:nx]) >= np.diag(H) + pr[:nx]), what
            ss.close()
            sd.close()


def host(t):
    return t.detach().cpu().numpy().copy()


def x_part_reference(s, v, w0, alpha, beta):
    """Rows [0, nx) of alpha K v + beta w0 in numpy.longdouble from the host copies, the same expression with absolute
    values (S) and the longest inner length per entry (L): the row's entries of H, the column's entries of A, and the
    three diagonal terms (reg, the two bound multipliers)."""
    st, nx, n, m = s.st, s.nx, s.st.n, s.st.m
    H, A = host(s.H.to_dense()).astype(LD), host(s.A.to_dense()).astype(LD)
    reg = host(st.reg)[:nx].astype(LD)
    vx, vy = v[:nx].astype(LD), v[n:n + m].astype(LD)
    vzl, vzu = v[n + m:n + m + st.nlb].astype(LD), v[n + m + st.nlb:].astype(LD)
    zl, zu = np.zeros(nx, dtype=LD), np.zeros(nx, dtype=LD)
    ilb, iub = host(st.ind_lb), host(st.ind_ub)
    zl[ilb[ilb < nx]] = vzl[ilb < nx]
    zu[iub[iub < nx]] = vzu[iub < nx]
    a, b = LD(alpha), LD(beta)
    E = a * (A.T @ vy) + a * (H @ vx) + a * reg * vx - a * zl + a * zu
    S = abs(a) * (np.abs(A.T) @ np.abs(vy) + np.abs(H) @ np.abs(vx) + np.abs(reg * vx) + np.abs(zl) + np.abs(zu))
    if beta != 0.0:
        E, S = E + b * w0[:nx].astype(LD), S + abs(b) * np.abs(w0[:nx]).astype(LD)
    L = np.count_nonzero(host(s.H.to_dense()), axis=1) + np.count_nonzero(host(s.A.to_dense()), axis=0) + 3
    return E, S, L


@pytest.mark.parametrize("form", ["condensed", "augmented"])
@pytest.mark.parametrize("nx", [1, 129, 300])
def test_mul_eval_and_solve(hip, nx, form):
    worst = 0.0
    for name in PATTERNS:
        ss, sd = built_pair(hip, nx, name, form, True)
        st, what = ss.st, (form, nx, name)
        n, m, ntot = st.n, st.m, st.ntot
        rng = np.random.default_rng(nx)
        v = rng.standard_normal(ntot)
        for alpha, beta in ((1.0, 0.0), (-1.0, 1.0), (0.5, -2.0)):
            w0 = np.full(ntot, np.nan) if beta == 0.0 else rng.standard_normal(ntot)
            out = []
            for s in (ss, sd):
                w = torch.as_tensor(w0.copy(), device=hip.device)
                s.kkt.mul(w, torch.as_tensor(v, device=hip.device), alpha, beta)
                out.append(host(w))
            E, S, L = x_part_reference(ss, v, w0, alpha, beta)
            err = np.abs(out[0][:nx].astype(LD) - E)
            assert np.all(np.isfinite(out[0][:nx])) and np.all(err <= (L + 4) * U * S), (what, alpha, beta, float(np.max(err / ((L + 4) * U * S))))
            worst = max(worst, float(np.max(err / np.maximum((L + 4) * U * S, LD(1e-300)))))
            assert np.array_equal(bits(out[0][n:]), bits(out[1][n:])), (what, alpha, beta)  # y, zl, zu: H does not enter
        # eval: f = H x + q, obj = c0 + q'x + x'Hx/2
        obj = ss.kkt.eval_model(ss.q, st.rhs, 0.25)
        H = host(ss.H.to_dense()).astype(LD)
        x, q = host(st.x)[:nx].astype(LD), host(ss.q).astype(LD)
        f_ref, f_S = H @ x + q, np.abs(H) @ np.abs(x) + np.abs(q)
        f_len = np.count_nonzero(host(ss.H.to_dense()), axis=1) + 1
        f = host(st.f)
        assert np.all(np.abs(f[:nx].astype(LD) - f_ref) <= (f_len + 4) * U * f_S) and not np.any(f[nx:]), what
        o_ref = LD(0.25) + q @ x + LD(0.5) * (x @ (H @ x))
        o_S = LD(0.25) + np.abs(q) @ np.abs(x) + LD(0.5) * (np.abs(x) @ (np.abs(H) @ np.abs(x)))
        assert abs(LD(obj) - o_ref) <= (ss.H.nnz + 2 * nx + 4) * U * o_S, (what, obj, float(o_ref))
        # solve!: K solve(b) = b
        b = rng.standard_normal(ntot)
        for s in (ss, sd):
            s.kkt.factorize_wrapper()
            assert s.kkt.linear_solver.is_factorized(), what
            s.st.p.copy_(torch.as_tensor(b))
            hip.copy(s.st.p, s.st.d)
            s.kkt.solve(s.st.d)
            hip.fill(0.0, s.st.w1)
            s.kkt.mul(s.st.w1, s.st.d, 1.0, 0.0)
            assert np.max(np.abs(host(s.st.w1) - b)) / np.max(np.abs(b)) < 1e-8, what
        ss.close()
        sd.close()
    print(f"mul! x-part, worst err / bound ({form}, nx={nx}): {worst:.3f}")


@functools.lru_cache(maxsize=None)
def oracle_runs(i):
    form, oname, seed, n, m, per_row, p, eq, _ = CASES[i]
    qp = sparse_hessian_qp(seed, n, m, per_row, p, eq)
    kw = dict(regularization=mpc.FixedRegularization(1e-8, -1e-8)) if form == "condensed" else {}
    return qp, mpc.solve(qp, kkt_system=oname, **kw), mpc.solve(qp, kkt_system=oname, refine_steps=1, **kw)


@pytest.mark.parametrize("i,driver", [(i, "python") for i in range(len(CASES))] + [(0, "native"), (3, "native")])
def test_whole_solves_vs_oracle(hip, i, driver):
    form, _, seed, n, m = CASES[i][:5]
    qp, ref, ref2 = oracle_runs(i)
    name = f"{form}-s{seed}-n{n}-m{m}-{driver}"
    assert ref["status"] == ref2["status"] == M.SOLVE_SUCCEEDED and ref["iter"] == ref2["iter"] == CASES[i][8], name
    kw = dict(regularization=REG) if form == "condensed" else {}
    s = M.MPCSolver(device_qp(qp, hip, M.DeviceSymCSR.from_dense(hip.device, qp.H)), hip, kkt_system=form, driver=driver, **kw)
    r = s.solve()
    assert isinstance(s.H, M.DeviceSymCSR) and type(s.kkt).__name__.startswith("HIPSparse")
    tol = s.opt.tol
    s.close()
    assert r["status"] == ref["status"], name
    assert parity.iteration_parity(r, ref, tol, name, lp=False) == "equal"
    parity.compare_traces_measured(r["trace"], ref["trace"], ref2["trace"], name)
    assert parity.close(r["objective"], ref["objective"], 1e-9), name
    assert np.max(np.abs(r["solution"] - ref["solution"])) <= 1e-7, name


def test_fixed_variables_as_parameters(hip):
    """make_parameter with a sparse H (``DeviceQP.eliminate_fixed``: q_free += H[free, fixed] x_fix, the constant, the
    submatrix) against the dense-H run of the same library."""
    qp = sparse_hessian_qp(11, 129, 40, 4, 1, equality_cons=(1,))
    fixed, vals = [107, 110, 115], [0.25, 0.39, 0.29]  # (about half their values at the optimum: the rest stays feasible)
    qp.lvar[fixed] = qp.uvar[fixed] = vals
    res = []
    for H in (M.DeviceSymCSR.from_dense(hip.device, qp.H), torch.as_tensor(qp.H, device=hip.device).contiguous()):
        s = M.MPCSolver(device_qp(qp, hip, H), hip, kkt_system="augmented", fixed_variable_treatment="make_parameter")
        res.append(s.solve())
        assert s.nx == 126 and type(s.qp.H) is type(H)
        s.close()
    a, b = res
    assert a["status"] == b["status"] == M.SOLVE_SUCCEEDED and a["iter"] == b["iter"]
    assert np.array_equal(a["solution"][fixed], vals)
    assert np.max(np.abs(a["solution"] - b["solution"])) <= 1e-9 * max(1.0, np.max(np.abs(b["solution"])))
    assert parity.close(a["objective"], b["objective"], 1e-9)
    for k in ("multipliers", "multipliers_L", "multipliers_U"):
        assert np.max(np.abs(a[k] - b[k])) <= 1e-6 * max(1.0, np.max(np.abs(b[k]))), k


def test_objective_scaling_reaches_the_stored_values(hip):
    """An objective 500 times as large: the gradient at the start exceeds 100, so ``obj_scale < 1`` and the library sees
    ``H.scaled(obj_scale)`` -- one product per stored value, the dense path's ``obj_scale * H`` -- and the same solve."""
    qp = sparse_hessian_qp(3, 100, 40, 6, 3)
    qp.q, qp.H = 500.0 * qp.q, 500.0 * qp.H
    res = []
    for H in (M.DeviceSymCSR.from_dense(hip.device, qp.H), torch.as_tensor(qp.H, device=hip.device).contiguous()):
        s = M.MPCSolver(device_qp(qp, hip, H), hip, regularization=REG)
        res.append(s.solve())
        assert s.obj_scale < 1.0
        if isinstance(H, M.DeviceSymCSR):
            assert s.H.col is H.col and np.array_equal(bits(host(s.H.val)), bits(host(H.val) * s.obj_scale))
        s.close()
    a, b = res
    assert a["status"] == b["status"] == M.SOLVE_SUCCEEDED and a["iter"] == b["iter"]
    assert parity.close(a["objective"], b["objective"], 1e-9)
    assert np.max(np.abs(a["solution"] - b["solution"])) <= 1e-9 * max(1.0, np.max(np.abs(b["solution"])))


def test_instance_file_keeps_its_hessian_sparse(hip, tmp_path):
    """QPS file with a non-diagonal Q -> read_qps -> presolve -> scale -> ``to_device(sparse_hessian=True)`` -> solve:
    H reaches the library as CSR (no n x n tensor on the way) and the solve is the dense-H path's."""
    from madqp_jl_amd import preprocess as P
    from tests.test_preprocess import planted_qp

    path = str(tmp_path / "planted.qps")
    P.write_qps(planted_qp(0), path)
    scaled = P.ruiz_scale(P.presolve(P.read_qps(path)).qp)[0]
    res = []
    for sparse_hessian in (True, False):
        dq = P.to_device(scaled, hip, sparse_hessian=sparse_hessian)
        assert isinstance(dq.H, M.DeviceSymCSR) == sparse_hessian and isinstance(dq.A, M.DeviceCSR)
        s = M.MPCSolver(dq, hip, kkt_system="augmented", tol=1e-9, driver="native")
        res.append(s.solve())
        assert isinstance(s.H, M.DeviceSymCSR) == sparse_hessian
        s.close()
    a, b = res
    assert dq.H.dim() == 2 and a["status"] == b["status"] == M.SOLVE_SUCCEEDED and a["iter"] == b["iter"]
    assert parity.close(a["objective"], b["objective"], 1e-9)
    assert np.max(np.abs(a["solution"] - b["solution"])) <= 1e-9 * max(1.0, np.max(np.abs(b["solution"])))


def test_abi_refusals_are_return_codes(hip):
    """Arguments are refused with MADQP_ERR_ARG through madqp_last_error; nothing is launched, the context stays usable."""
    nx, m = 6, 3
    dev = hip.device
    A = np.zeros((m, nx))
    A[0, 0], A[1, 2], A[2, 5], A[2, 1] = 1.0, -2.0, 0.5, 3.0
    csr = M.DeviceCSR.from_dense(dev, A)
    t_val = csr.t_val
    Ad = torch.as_tensor(A, device=dev).contiguous()
    h = M.DeviceSymCSR.from_dense(dev, np.eye(nx) + np.diag(np.full(nx - 1, 0.25), -1))
    Hd = h.to_dense().contiguous()
    hdiag = torch.ones(nx, dtype=torch.float64, device=dev)
    made = []

    def sparse(mode, H=None):
        made.append(hip.kkt_create_sparse(mode, nx, m, [0, 2], H, nx, csr, t_val))
        return made[-1]

    def refused(handle):
        with pytest.raises(M.MadQPError, match=r"error -1: bad argument"):
            hip.kkt_set_hcsr(handle, h)

    refused(sparse(0, Hd))  # a dense H is held
    k = sparse(2)
    hip.kkt_set_hdiag(k, hdiag)
    refused(k)  # a diagonal H is held
    refused(sparse(1))  # normal equations
    made.append(hip.kkt_create(nx, m, [0, 2], None, nx, Ad, nx))
    refused(made[-1])  # dense Jacobian
    for create in (hip.kkt_create_augmented, hip.kkt_create_scaled_augmented):
        made.append(create(nx, m, [0, 2], None, nx, Ad, nx))
        refused(made[-1])
    with pytest.raises(M.MadQPError, match=r"error -1: bad argument"):  # a null h_ptr
        hip._ck(hip.lib.madqp_kkt_set_hcsr(sparse(0), None, None, None))
    # the context is usable: the call succeeds where it is served, and the diagonal form is refused after it
    for mode in (0, 2):
        k = sparse(mode)
        hip.kkt_set_hcsr(k, h)
        with pytest.raises(M.MadQPError, match=r"error -1: bad argument"):
            hip.kkt_set_hdiag(k, hdiag)
    empty = M.DeviceSymCSR(dev, nx, [], [], [])
    hip._ck(hip.lib.madqp_kkt_set_hcsr(sparse(0), M._lib.ptr(empty.ptr), None, None))  # nnz = 0: no col / val needed
    hip.sync()
    for k in made:
        hip.kkt_destroy(k)
