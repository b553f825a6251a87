"""Helpers of tests/test_gpu_gemm_paths.py: one product through the seam madqp_debug_gemm_tn, its references, and the
checks every case shares.  Run as a script it is the child process of the environment-knob variants:

    python tests/gemm_paths.py NAME [NAME ...]     ->  one JSON line {NAME: {"sha": .., "info": .., "ratio": ..}}

Layout (csrc/common.h, GemmArgs): X[i + k*ldx], Y[j + k*ldy], C[i + j*ldc] -- on the host X is an array (K, ldx), Y an
array (K, ldy) and C an array (N, ldc) whose row j is column j of the product.

Tolerance (derived, not measured).  With S = |alpha| (|X| |Y|^T) + |beta| |Cin| + |dvec| elementwise and u = 2^-53, any
order of summation, with or without FMA, split in K or not, satisfies |out - exact| <= (K + 4) u S (Higham, Accuracy and
Stability of Numerical Algorithms, sec. 3.1).  So every written entry is held to 2 (K + 4) u S against the float64 numpy
product (which carries the same bound), and a sample -- every entry of a small case -- to (K + 4) u S against a reference
in numpy.longdouble (x87 extended, eps 2^-63: its own error is 2^-11 of the bound) or, where longdouble is no wider than
that, in exact rational arithmetic."""
import ctypes as C
import hashlib
import json
import os
import sys
from fractions import Fraction

import numpy as np
import torch

U = 2.0 ** -53
T = 128  # tile edge
LD_OK = float(np.finfo(np.longdouble).eps) < 2.0 ** -60
INFO_FIELDS = ("ntiles", "ksplit", "kchunk", "tail_tiles", "tail_split", "segments", "persistent_workgroups", "fast_ok",
               "batch_xcd", "gemm_slots")


def even_above(n, extra):
    return (n + extra + 1) // 2 * 2


class Problem:
    """Seeded asymmetric operands of one product (X != Y unless y_is_x), with the addend / diagonal the case asks for.
    Leading dimensions exceed the extents; the padding of the operands holds finite garbage."""

    def __init__(self, seed, M, N, K, *, lower=0, diag_off=0, alpha=1.0, beta=1.0, cin="none", dvec=False, Mread=0,
                 Nread=0, ldx=None, ldy=None, y_is_x=False):
        rng = np.random.default_rng(seed)
        self.M, self.N, self.K = M, N, K
        self.lower, self.diag_off, self.alpha, self.beta = lower, diag_off, float(alpha), float(beta)
        self.Mread, self.Nread = Mread, Nread
        self.ldx = ldx or even_above(max(M, Mread, 1), 6)
        self.ldy = ldy or even_above(max(N, Nread, 1), 10)
        ks = max(K, 1)  # (K = 0: one row of storage so that the pointers are not null)
        self.X = rng.standard_normal((ks, self.ldx))
        self.Y = self.X if y_is_x else rng.standard_normal((ks, self.ldy))
        if y_is_x:
            assert M == N
            self.ldy = self.ldx
        self.ldc = M + 5
        self.cin = cin  # "none" | "sep" (own array, ldcin != ldc) | "alias" (Cin == C)
        self.ldcin = self.ldc if cin == "alias" else M + 3
        self.Cin = rng.standard_normal((max(N, 1), self.ldcin)) if cin != "none" else None
        self.dvec = rng.uniform(1.0, 2.0, max(N, 1)) * rng.choice([-1.0, 1.0], max(N, 1)) if dvec else None

    # ---- what the call may write -------------------------------------------------------------------------------
    def written(self, cols=None, tile_row0=None):
        i = np.arange(self.M)[:, None]
        j = np.arange(self.N)[None, :]
        W = np.ones((self.M, self.N), dtype=bool)
        if self.lower:
            W &= (i + self.diag_off >= j)
        if cols is not None:
            on = np.zeros(self.N, dtype=bool)
            for a, b in zip(cols[0::2], cols[1::2]):
                on[a:b] = True
            W &= on[None, :]
        if tile_row0 is not None:
            W &= (i // T >= np.asarray(tile_row0)[j // T])
        return W

    def prior(self, W):
        """C before the call: NaN everywhere, except the addend where Cin aliases C and the call may write."""
        P = np.full((max(self.N, 1), self.ldc), np.nan)
        if self.cin == "alias":
            P[:self.N, :self.M][W.T] = self.Cin[:self.N, :self.M][W.T]
        return P

    # ---- references --------------------------------------------------------------------------------------------
    def reference(self):
        """(ref, S) in float64, M x N."""
        M, N, K = self.M, self.N, self.K
        Xm, Ym = self.X[:K, :M], self.Y[:K, :N]
        ref = self.alpha * (Xm.T @ Ym)
        S = abs(self.alpha) * (np.abs(Xm).T @ np.abs(Ym))
        if self.Cin is not None:
            ref = ref + self.beta * self.Cin[:N, :M].T
            S = S + abs(self.beta) * np.abs(self.Cin[:N, :M].T)
        if self.dvec is not None:
            j = np.arange(N)
            i = j - self.diag_off
            ok = (i >= 0) & (i < M)
            ref[i[ok], j[ok]] += self.dvec[j[ok]]
            S[i[ok], j[ok]] += np.abs(self.dvec[j[ok]])
        return ref, S

    def reference_wide(self, ii, jj):
        """(ref, S) at the entries (ii, jj) in extended precision (longdouble, or exact rationals rounded once)."""
        K = self.K
        ref = np.zeros(len(ii), dtype=np.longdouble)
        S = np.zeros(len(ii), dtype=np.longdouble)
        if not LD_OK:
            return self._reference_exact(ii, jj)
        step = max(1, 4_000_000 // max(K, 1))
        for a in range(0, len(ii), step):
            i, j = ii[a:a + step], jj[a:a + step]
            xs = self.X[:K, i].astype(np.longdouble)
            ys = self.Y[:K, j].astype(np.longdouble)
            ref[a:a + step] = np.longdouble(self.alpha) * (xs * ys).sum(axis=0)
            S[a:a + step] = np.longdouble(abs(self.alpha)) * (np.abs(xs) * np.abs(ys)).sum(axis=0)
        if self.Cin is not None:
            c = self.Cin[jj, ii].astype(np.longdouble)
            ref += np.longdouble(self.beta) * c
            S += np.longdouble(abs(self.beta)) * np.abs(c)
        if self.dvec is not None:
            d = np.where(ii + self.diag_off == jj, self.dvec[jj], 0.0).astype(np.longdouble)
            ref += d
            S += np.abs(d)
        return ref, S

    def _reference_exact(self, ii, jj):
        ref = np.zeros(len(ii))
        S = np.zeros(len(ii))
        F = Fraction
        for n, (i, j) in enumerate(zip(ii, jj)):
            acc = sum((F(float(x)) * F(float(y)) for x, y in zip(self.X[:self.K, i], self.Y[:self.K, j])), F(0))
            sab = sum((abs(F(float(x)) * F(float(y))) for x, y in zip(self.X[:self.K, i], self.Y[:self.K, j])), F(0))
            r, s = F(self.alpha) * acc, abs(F(self.alpha)) * sab
            if self.Cin is not None:
                r += F(self.beta) * F(float(self.Cin[j, i]))
                s += abs(F(self.beta) * F(float(self.Cin[j, i])))
            if self.dvec is not None and i + self.diag_off == j:
                r += F(float(self.dvec[j]))
                s += abs(F(float(self.dvec[j])))
            ref[n], S[n] = float(r), float(s)
        return ref, S


def dev(a, be, shift=0):
    """Device copy of a host array; shift = 1: at an address 8 bytes past a 16-byte boundary."""
    a = np.ascontiguousarray(a, dtype=np.float64).ravel()
    buf = torch.empty(a.size + 2, dtype=torch.float64, device=be.device)
    base = 0 if (buf.data_ptr() % 16 == 0) else 1  # (torch allocations are 256-byte aligned; be explicit anyway)
    t = buf[base + shift:base + shift + a.size]
    t.copy_(torch.from_numpy(a))
    assert t.data_ptr() % 16 == 8 * shift
    return t


def i32dev(a, be):
    return torch.as_tensor(np.asarray(a, dtype=np.int32), device=be.device)


def seam(be, **f):
    """One madqp_debug_gemm_tn.  Fields by name; tensors for device pointers, sequences for the two host arrays.
    Returns (return code, info dict).  The call is asynchronous: read results through torch (same stream)."""
    from madqp_jl_amd._lib import CDebugGemm, CDebugGemmInfo

    a = CDebugGemm()
    keep = []
    for k, v in f.items():
        if k in ("tile_row0_host", "cols_host"):
            if v is not None:
                arr = (C.c_int64 * len(v))(*[int(x) for x in v])
                keep.append(arr)
                v = C.cast(arr, C.POINTER(C.c_int64))
        elif isinstance(v, torch.Tensor):
            keep.append(v)
            v = v.data_ptr()
        setattr(a, k, v)
    info = CDebugGemmInfo()
    rc = be.lib.madqp_debug_gemm_tn(be.ctx, C.byref(a), C.byref(info))
    return rc, {k: int(getattr(info, k)) for k in INFO_FIELDS}


def run(be, p, *, cols=None, tile_row0=None, cap_slots=0, shift=0, prior=None):
    """Problem p through the seam.  Returns (rc, info, C after the call as a host array (N, ldc), C before it)."""
    W = p.written(cols, tile_row0)
    P = p.prior(W) if prior is None else prior
    Cd = dev(P, be)
    Xd = dev(p.X, be, shift)
    Yd = Xd if p.Y is p.X else dev(p.Y, be, shift)
    f = dict(X=Xd, ldx=p.ldx, Y=Yd, ldy=p.ldy, C=Cd, ldc=p.ldc, alpha=p.alpha, beta=p.beta, M=p.M, N=p.N, K=p.K,
             Mread=p.Mread, Nread=p.Nread, diag_off=p.diag_off, lower_only=p.lower, cap_slots=cap_slots)
    if p.cin == "alias":
        f.update(Cin=Cd, ldcin=p.ldc)
    elif p.cin == "sep":
        f.update(Cin=dev(p.Cin, be), ldcin=p.ldcin)
    if p.dvec is not None:
        f.update(dvec=dev(p.dvec, be))
    if cols is not None:
        f.update(cols_host=list(cols), ncols=len(cols) // 2)
    if tile_row0 is not None:
        f.update(tile_row0_host=list(tile_row0))
    rc, info = seam(be, **f)
    out = Cd.cpu().numpy().reshape(P.shape)
    return rc, info, out, P


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def sample_entries(p, W):
    """The four corners and one interior point of every output tile, the rows and columns at M - 1 and N - 1 and the
    entries with i + diag_off == j -- those of them the call writes."""
    M, N = p.M, p.N
    ii, jj = [], []
    for tm in range((M + T - 1) // T):
        i0, i1 = tm * T, min(tm * T + T, M) - 1
        for tn in range((N + T - 1) // T):
            j0, j1 = tn * T, min(tn * T + T, N) - 1
            ii += [i0, i0, i1, i1, min(i0 + 53, i1)]
            jj += [j0, j1, j0, j1, min(j0 + 77, j1)]
    ii += [M - 1] * N + list(range(M))
    jj += list(range(N)) + [N - 1] * M
    d = np.arange(N)
    ok = (d - p.diag_off >= 0) & (d - p.diag_off < M)
    ii += list(d[ok] - p.diag_off)
    jj += list(d[ok])
    ii, jj = np.asarray(ii, dtype=np.int64), np.asarray(jj, dtype=np.int64)
    keep = W[ii, jj]
    key = np.unique(ii[keep] * N + jj[keep])
    return key // N, key % N


def explain(p, out, ref, i, j, info):
    """Where the worst entry lies, and -- for a split launch -- which chunk of K its difference looks like."""
    d = float(out[i, j] - ref[i, j])
    msg = (f"entry ({i}, {j}) of tile ({i // T}, {j // T}): out {out[i, j]!r} ref {ref[i, j]!r} diff {d:.3e}; "
           f"dispatch {info}")
    kc = info.get("kchunk", 0)
    if (info.get("ksplit", 1) > 1 or info.get("tail_tiles", 0) > 0) and kc > 0 and np.isfinite(d) and d != 0.0:
        parts = [p.alpha * float(p.X[k0:min(k0 + kc, p.K), i] @ p.Y[k0:min(k0 + kc, p.K), j]) for k0 in range(0, p.K, kc)]
        c = int(np.argmin([abs(d + q) for q in parts]))
        if abs(d + parts[c]) <= 1e-6 * abs(d):
            msg += f"; the difference is minus the partial sum of K-chunk {c} (k in [{c * kc}, {min((c + 1) * kc, p.K)}))"
        c2 = int(np.argmin([abs(d - q) for q in parts]))
        if abs(d - parts[c2]) <= 1e-6 * abs(d):
            msg += f"; the difference is the partial sum of K-chunk {c2} counted twice"
    return msg


def check(p, out_full, prior_full, info, label, *, cols=None, tile_row0=None, full=True):
    """Every assertion a case shares; returns (worst err / bound against float64, against the wide reference)."""
    M, N, K = p.M, p.N, p.K
    W = p.written(cols, tile_row0)
    Wf = np.zeros(out_full.shape, dtype=bool)
    Wf[:N, :M] = W.T
    # not written means not written: the bits C held before the call
    a, b = out_full.view(np.uint64), prior_full.view(np.uint64)
    touched = (a != b) & ~Wf
    if touched.any():
        j, i = np.argwhere(touched)[0]
        raise AssertionError(f"{label}: {int(touched.sum())} entries outside what the call may write were changed, the first "
                             f"at row {i}, column {j} (tile ({i // T}, {j // T}), M = {M}, N = {N}, ldc = {p.ldc}): "
                             f"{prior_full[j, i]!r} -> {out_full[j, i]!r}; dispatch {info}")
    out = out_full[:N, :M].T
    r64 = rld = 0.0
    if full and W.any():
        ref, S = p.reference()
        err = np.abs(out - ref)
        bound = 2.0 * (K + 4) * U * S
        bad = W & ~(err <= bound)
        if bad.any():
            q = np.where(bad, np.where(np.isfinite(err), err / np.maximum(bound, 1e-300), np.inf), -1.0)
            i, j = np.unravel_index(int(np.argmax(q)), q.shape)
            tiles = [(int(x), int(y)) for x, y in np.unique(np.argwhere(bad) // T, axis=0)]
            raise AssertionError(f"{label}: {int(bad.sum())} entries beyond 2 (K + 4) u S against float64 in tiles {tiles[:12]}"
                                 f"{' ..' if len(tiles) > 12 else ''}; worst: " + explain(p, out, ref, i, j, info))
        nz = W & (bound > 0)
        r64 = float(np.max(err[nz] / bound[nz])) if nz.any() else 0.0
    if W.any():
        if M * N * max(K, 1) <= 30_000_000:
            ii, jj = np.nonzero(W)
        else:
            ii, jj = sample_entries(p, W)
        ref, S = p.reference_wide(ii, jj)
        err = np.abs(out[ii, jj].astype(np.longdouble) - ref)
        bound = np.longdouble((K + 4) * U) * S
        bad = ~(err <= bound)
        if bad.any():
            q = np.where(np.isfinite(err), err / np.maximum(bound, np.longdouble(1e-300)), np.inf)
            n = int(np.argmax(np.where(bad, q, -1.0)))
            dense = np.full((M, N), np.nan)
            dense[ii, jj] = ref.astype(np.float64)
            raise AssertionError(f"{label}: {int(bad.sum())} of {len(ii)} sampled entries beyond (K + 4) u S against the "
                                 f"extended-precision reference; worst: " + explain(p, out, dense, int(ii[n]), int(jj[n]), info))
        nz = bound > 0
        rld = float(np.max(err[nz] / bound[nz])) if nz.any() else 0.0
    print(f"[gemm-paths] {label}: M {M} N {N} K {K} err/bound {r64:.3e} (float64, bound 2(K+4)uS) {rld:.3e} (extended, "
          f"bound (K+4)uS) {info}")
    return r64, rld


# ---- the launches whose variants need a process of their own (the environment knobs are read once per process) ----------
CHILD_CASES = {
    # name: (M, N, K, lower)
    "seg2": (5000, 5000, 512, 1),       # 820 tiles: MADQP_GEMM_SEG_ROUNDS=1 -> segments 512 + 308
    "seg5": (9000, 9000, 64, 1),        # 2556 tiles: five segments, the last one 508
    "seg_merge": (5888, 5888, 64, 1),   # 1081 tiles = 2 x 512 + 57: the short rest joins the second segment
    "split": (1000, 1000, 5000, 1),     # few tiles: split-K
    "tail": (4000, 4000, 1024, 1),      # 528 tiles: 512 whole + 16 tail tiles cut in K
}


def child_case(be, name):
    M, N, K, lower = CHILD_CASES[name]
    p = Problem(sum(map(ord, name)) * 1000 + K, M, N, K, lower=lower, cin="sep", dvec=True)
    rc, info, out, prior = run(be, p)
    assert rc == 0, (name, rc)
    r64, rld = check(p, out, prior, info, name)
    return {"sha": sha(out), "info": info, "ratio": [r64, rld]}


def main(names):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    if root not in sys.path:
        sys.path.insert(0, root)
    import madqp_jl_amd as M

    be = M.HipBackend(0)
    try:
        res = {n: child_case(be, n) for n in names}
    finally:
        be.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main(sys.argv[1:])
