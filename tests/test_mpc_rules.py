"""The result-block layout and the scalar rules of an interior-point iteration (madqp_jl_amd/csrc/mpc_rules.inc, compiled for the
CPU by tests/csrc): the functions both native drivers call -- the host driver (csrc/mpc.hip) with its one-thread kernels
(csrc/vec_kernels.hip), and the batched engine (csrc/batch_wg.inc) -- held to the arithmetic of oracle/mpc.py bit for bit, to
explicit figures on both sides of every constant and branch, and to the oracle on non-finite operands.  No GPU."""
import ctypes as C
import math
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f64 = np.float64
NAN, INF = f64("nan"), f64("inf")
pd = C.POINTER(C.c_double)


@pytest.fixture(scope="module")
def lib():
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "tests", "csrc")], stdout=subprocess.DEVNULL)
    lib = C.CDLL(os.path.join(ROOT, "tests", "_build", "libmadqp_mpc_rules.so"))
    lib.mpc_layout_c.argtypes = [C.c_int, C.POINTER(C.c_char_p), C.POINTER(C.c_int), C.POINTER(C.c_int)]
    lib.mpc_read_counts_c.argtypes = [C.POINTER(C.c_int)]
    lib.mpc_verdict_c.argtypes = [pd, C.c_int, C.c_double, pd]
    lib.mpc_steps_c.argtypes = [pd, pd]
    lib.mpc_barrier_block_c.argtypes = [pd, C.c_double, C.c_double, C.c_int, C.c_double, pd]
    lib.mpc_trial_alpha_block_c.argtypes = [pd, pd]
    lib.mpc_muc_c.argtypes = [pd, C.c_double, C.c_double]
    lib.mpc_muc_c.restype = C.c_double
    lib.mpc_trial_dropped_c.argtypes = [pd, pd]
    lib.mpc_decide_c.argtypes = [pd, C.c_int, C.c_int, C.c_int, C.c_double, pd]
    return lib


def arr(v):
    a = np.ascontiguousarray(v, dtype=np.float64)
    return a, a.ctypes.data_as(pd)


def same_bits(a, b):
    return np.array_equal(np.asarray(a, dtype=np.float64).view(np.uint64), np.asarray(b, dtype=np.float64).view(np.uint64))


@pytest.fixture(scope="module")
def layout(lib):
    """name -> (first, width): the fields, the parts of the trial block at both bases, the later trials' sums."""
    name, first, width = C.c_char_p(), C.c_int(), C.c_int()
    n = lib.mpc_layout_c(-1, C.byref(name), C.byref(first), C.byref(width))
    rows = {}
    for i in range(n):
        lib.mpc_layout_c(i, C.byref(name), C.byref(first), C.byref(width))
        rows[name.value.decode()] = (first.value, width.value)
    assert len(rows) == n
    return rows


@pytest.fixture(scope="module")
def counts(lib):
    out = (C.c_int * 5)()
    lib.mpc_read_counts_c(out)
    return dict(zip(("corrector", "first_trial", "decision", "later_trial", "final"), out))


# ---- layout -------------------------------------------------------------------------------------------------------------
def test_fields_do_not_overlap_and_end_below_the_fault_word(lib, layout):
    text = open(os.path.join(ROOT, "madqp_jl_amd", "csrc", "common.h")).read()
    slots = int(re.search(r"#define MADQP_RESULT_SLOTS (\d+)", text).group(1))
    fault = lib.mpc_fault_slot_c()
    assert fault == slots - 1  # the test build's constant is the library's
    fields = {k: v for k, v in layout.items() if "." not in k and k != "LATER_COMPL"}
    assert set(fields) == {"PRED_NRM", "PRED_ALPHA", "COMPL", "INFO", "BARRIER", "CORR_NRM", "CORR_ALPHA", "CORR_DNORM",
                           "GZ_ALPHA", "MUC", "TRIAL_ALPHA", "TRIAL_COMPL", "TRIAL", "DECISION", "PHASE_C"}
    used = np.zeros(slots, dtype=int)
    for first, width in fields.values():
        assert width > 0 and 0 <= first and first + width <= fault
        used[first:first + width] += 1
    assert used.max() == 1
    # what the kernels behind each field write: 3 norms, 8 step-length words, 2 sums each, 2 + 4 words behind the update
    widths = {k: w for k, (_, w) in fields.items()}
    assert widths == dict(PRED_NRM=3, PRED_ALPHA=8, COMPL=4, INFO=1, BARRIER=3, CORR_NRM=3, CORR_ALPHA=8, CORR_DNORM=3,
                          GZ_ALPHA=8, MUC=1, TRIAL_ALPHA=8, TRIAL_COMPL=2, TRIAL=22, DECISION=4, PHASE_C=6)


def test_each_read_back_covers_what_the_host_reads_from_it(lib, layout, counts):
    end = lambda k: sum(layout[k])
    corrector = ("PRED_NRM", "INFO", "BARRIER", "CORR_NRM", "CORR_ALPHA", "CORR_DNORM")
    assert counts["corrector"] >= max(map(end, corrector))
    assert counts["first_trial"] >= max(map(end, corrector + ("GZ_ALPHA", "TRIAL")))
    assert counts["decision"] >= max(map(end, corrector + ("GZ_ALPHA", "TRIAL", "DECISION")))
    assert counts["later_trial"] >= max(end("LATER." + p) for p in ("nrm", "alpha_gz", "alpha_tau", "dnorm"))
    assert counts["final"] >= end("PHASE_C")
    assert all(c < lib.mpc_fault_slot_c() for c in counts.values())  # (madqp_read_results refuses a count that reaches the fault word)
    assert counts == dict(corrector=49, first_trial=96, decision=104, later_trial=22, final=112)  # no word more than before


def test_trial_block_is_the_same_at_both_bases(layout):
    parts = ("nrm", "alpha_gz", "alpha_tau", "dnorm")
    first = [(layout["TRIAL." + p][0] - layout["TRIAL"][0], layout["TRIAL." + p][1]) for p in parts]
    later = [(layout["LATER." + p][0] - layout["LATER.nrm"][0], layout["LATER." + p][1]) for p in parts]
    assert first == later == [(0, 3), (3, 8), (11, 8), (19, 3)]
    assert sum(first[-1]) == layout["TRIAL"][1]
    # a later trial runs when the host has read the block, but mu_curr, tau and mu_c are still read on the device
    later_end = max(sum(layout["LATER." + p]) for p in parts)
    assert max(later_end, sum(layout["LATER_COMPL"])) <= min(layout["BARRIER"][0], layout["MUC"][0])


# ---- update_barrier! ------------------------------------------------------------------------------------------------------
def ref_barrier(sums, nb, mu_min, step_rule, step_param):
    """oracle/mpc.py: get_(affine_)complementarity_measure's mean, update_barrier, and update_step's tau."""
    s = [f64(v) for v in sums]
    with np.errstate(all="ignore"):
        mu_affine = (s[0] + s[1]) / nb if nb > 0 else 0.0
        mu_curr = (s[2] + s[3]) / nb if nb > 0 else 0.0
        if nb > 0:
            t = mu_affine / mu_curr
            sigma = min(max(t * t * t, 1e-6), 10.0)
        else:
            sigma = 1.0
        mu = max(mu_min, sigma * mu_curr)
        tau = step_param if step_rule == 0 else max(1 - mu, step_param)
    return [mu, tau, mu_curr]


def barrier(lib, sums, nb, mu_min, step_rule, step_param):
    _, ps = arr(sums)
    out, po = arr(np.zeros(3))
    lib.mpc_barrier_block_c(ps, float(nb), mu_min, step_rule, step_param, po)
    return out


def test_barrier_update_is_bitwise_the_oracles(lib):
    rng = np.random.default_rng(20250614)
    for _ in range(400):
        nb = int(rng.integers(1, 5000))
        curr = rng.uniform(0.0, 1.0, 2) * 10.0 ** rng.uniform(-12, 3) * nb
        aff = curr * rng.uniform(0.0, 2.5, 2)  # t^3 from 0 to ~15: all three branches of the clamp
        mu_min = 10.0 ** rng.uniform(-14, -6)
        param = float(rng.choice([0.99, 0.995, 0.9]))
        for rule in (0, 1):
            sums = np.concatenate([aff, curr])
            assert same_bits(barrier(lib, sums, nb, mu_min, rule, param), ref_barrier(sums, nb, mu_min, rule, param))


def test_barrier_update_on_both_sides_of_its_constants(lib):
    nb, mu_min = 4, 1e-11
    for t, sigma in ((0.0099, 1e-6), (0.0101, 0.0101 * 0.0101 * 0.0101), (2.154, 2.154 * 2.154 * 2.154), (2.155, 10.0),
                     (0.0, 1e-6), (1.0, 1.0)):
        mu_curr = 0.5
        sums = [t * mu_curr * nb, 0.0, mu_curr * nb, 0.0]
        assert f64(sums[0]) / nb / mu_curr == t  # (the figures above are what the rule sees)
        got = barrier(lib, sums, nb, mu_min, 1, 0.99)
        assert same_bits(got, ref_barrier(sums, nb, mu_min, 1, 0.99))
        assert same_bits(got, [sigma * mu_curr, max(1 - sigma * mu_curr, 0.99), mu_curr]), (t, got)
    assert 0.0099 ** 3 < 1e-6 < 0.0101 ** 3 and 2.154 ** 3 < 10.0 < 2.155 ** 3
    # mu_min wins, from either side; tau of ConservativeStep is its parameter, of AdaptiveStep max(1 - mu, tau_min)
    assert same_bits(barrier(lib, [4e-12, 0, 4e-12, 0], 4, 1e-11, 0, 0.99), [1e-11, 0.99, 1e-12])
    assert same_bits(barrier(lib, [4e-10, 0, 4e-10, 0], 4, 1e-11, 1, 0.99), [1e-10, 1 - 1e-10, 1e-10])
    assert same_bits(barrier(lib, [0.4, 0, 0.4, 0], 4, 1e-11, 1, 0.99), [0.1, 0.99, 0.1])
    assert same_bits(barrier(lib, [0.04, 0, 0.04, 0], 4, 1e-11, 1, 0.99), [0.01, 0.99, 0.01])  # 1 - mu == tau_min
    assert same_bits(barrier(lib, [0.04, 0, 0.04, 0], 4, 1e-11, 0, 0.5), [0.01, 0.5, 0.01])
    # no bound at all: both means are 0 without a division, sigma = 1
    for rule in (0, 1):
        assert same_bits(barrier(lib, [0, 0, 0, 0], 0, 1e-11, rule, 0.99), [1e-11, (0.99, 1 - 1e-11)[rule], 0.0])
        assert same_bits(barrier(lib, [0, 0, 0, 0], 0, 1e-11, rule, 0.99), ref_barrier([0, 0, 0, 0], 0, 1e-11, rule, 0.99))
    # a NaN goes the way of min / max as the oracle (and std::min / std::max) write them: sigma and sigma * mu_curr are
    # NaN, and max(mu_min, NaN) is mu_min
    for sums in ([NAN, 0, 2.0, 0], [1.0, 0, NAN, 0], [0.0, 0, 0.0, 0], [INF, 0, 1.0, 0]):
        got = barrier(lib, sums, 4, 1e-11, 1, 0.99)
        assert same_bits(got, ref_barrier(sums, 4, 1e-11, 1, 0.99)), (sums, got)
    assert same_bits(barrier(lib, [NAN, 0, 2.0, 0], 4, 1e-11, 1, 0.99), [1e-11, 1 - 1e-11, 0.5])


# ---- solve_system!'s verdict ------------------------------------------------------------------------------------------------
def verdict(lib, nrm, check, tol):
    _, pn = arr(nrm)
    ratio = C.c_double()
    bad = lib.mpc_verdict_c(pn, int(check), tol, C.byref(ratio))
    return bool(bad), ratio.value


def ref_failed(nrm, check, tol):  # oracle/mpc.py:683-688
    with np.errstate(invalid="ignore"):
        ratio = f64(nrm[0]) / max(1.0, f64(nrm[1]))
    return bool(math.isnan(ratio) or (check and ratio > tol)), ratio


def test_residual_verdict(lib):
    tol = 1e-8
    above = float(np.nextafter(tol, 1.0))
    assert verdict(lib, [tol, 1.0, 7.0], True, tol) == (False, tol)        # exactly at the tolerance: passes
    assert verdict(lib, [above, 1.0, 7.0], True, tol) == (True, above)     # one ulp above: SolveException
    assert verdict(lib, [above, 1.0, 7.0], False, tol) == (False, above)   # check_residual off
    assert verdict(lib, [1e300, 1.0, 7.0], False, tol) == (False, 1e300)
    assert verdict(lib, [INF, 1.0, 7.0], False, tol) == (False, INF)
    for nrm in ([NAN, 1.0, 0.0], [1.0, NAN, 0.0], [INF, INF, 0.0]):       # NaN fails with the check off too;
        bad, ratio = verdict(lib, nrm, False, tol)                         # max(1.0, NaN) is 1.0, as the oracle's
        assert (bad, math.isnan(ratio)) == (ref_failed(nrm, False, tol)[0], math.isnan(ref_failed(nrm, False, tol)[1]))
    assert verdict(lib, [NAN, 1.0, 0.0], False, tol)[0] and verdict(lib, [INF, INF, 0.0], True, tol)[0]
    assert verdict(lib, [1.0, NAN, 0.0], False, tol) == (False, 1.0)
    assert verdict(lib, [5e-9, 0.25, 7.0], True, tol) == (False, 5e-9)     # |p| < 1: the denominator is 1,
    assert verdict(lib, [5e-9, 4.0, 7.0], True, tol) == (False, 1.25e-9)   # not |p|
    assert verdict(lib, [3e-8, 4.0, 7.0], True, tol) == (False, 7.5e-9) and verdict(lib, [3e-8, 2.0, 7.0], True, tol)[0]
    rng = np.random.default_rng(3)
    for _ in range(200):
        nrm = 10.0 ** rng.uniform(-12, 2, 3)
        for check in (False, True):
            assert verdict(lib, nrm, check, tol) == ref_failed(nrm, check, tol)


# ---- Gondzio's trial: step lengths, mu_c, keep or drop ------------------------------------------------------------------------
def block8(ap0, ap1, ad0, ad1):
    """(value, index) of {xl, xu, zl, zu} as alpha_max_final_kernel leaves them."""
    return [ap0, 11.0, ap1, 12.0, ad0, 13.0, ad1, 14.0]


def steps(lib, a8):
    _, pa = arr(a8)
    out, po = arr(np.zeros(2))
    lib.mpc_steps_c(pa, po)
    return out


def test_step_length_combine_and_its_ties(lib):
    assert same_bits(steps(lib, block8(0.3, 0.7, 0.9, 0.2)), [0.3, 0.2])
    assert same_bits(steps(lib, block8(0.5, 0.5, 1.0, 1.0)), [0.5, 1.0])
    assert same_bits(steps(lib, block8(0.0, -0.0, -0.0, 0.0)), [min(0.0, -0.0), min(-0.0, 0.0)])  # the first of a tie
    assert same_bits(steps(lib, block8(0.0, -0.0, -0.0, 0.0)), [0.0, -0.0])
    assert same_bits(steps(lib, block8(NAN, 0.5, 0.5, NAN)), [min(NAN, f64(0.5)), min(f64(0.5), NAN)])


def test_trial_alpha_above_at_and_below_one(lib):
    for ap, ad in ((0.95, 0.5), (0.9, 0.9000000000000001), (0.8999999999999999, 0.0), (1.0, 0.3), (0.25, 0.75)):
        out, po = arr(np.full(8, -7.0))
        lib.mpc_trial_alpha_block_c(arr(block8(ap, 1.0, 1.0, ad))[1], po)
        tp, td = min(ap + 0.1, 1.0), min(ad + 0.1, 1.0)  # oracle/mpc.py:800
        assert same_bits(out, [tp, -7.0, tp, -7.0, td, -7.0, td, -7.0])
        assert same_bits(steps(lib, out), [tp, td])  # the readers of the 8-slot pattern get them back
    assert min(0.95 + 0.1, 1.0) == 1.0 and 0.9 + 0.1 == 1.0 and 0.8999999999999999 + 0.1 < 1.0


def test_mu_c_is_bitwise_the_oracles(lib):
    rng = np.random.default_rng(5)
    for _ in range(300):
        nb = int(rng.integers(1, 3000))
        sums = rng.uniform(0.0, 1.0, 2) * 10.0 ** rng.uniform(-10, 2) * nb
        mu_curr = f64(10.0 ** rng.uniform(-10, 2))
        ga = (f64(sums[0]) + f64(sums[1])) / nb
        r = ga / mu_curr
        assert same_bits(lib.mpc_muc_c(arr(sums)[1], float(nb), mu_curr), r * r * ga)  # (ga / mu_curr) ** 2 * ga
    assert lib.mpc_muc_c(arr([0.0, 0.0])[1], 0.0, 1.0) == 0.0  # no bound: the mean is 0 without a division


def dropped(lib, trial, before):
    return bool(lib.mpc_trial_dropped_c(arr(trial)[1], arr(before)[1]))


def test_keep_or_drop(lib):
    ap, ad = 0.6180339887, 0.4142135623
    thr_p, thr_d = 1.005 * ap, 1.005 * ad
    below = lambda v: float(np.nextafter(v, 0.0))
    assert not dropped(lib, [thr_p, thr_d], [ap, ad])         # ha == 1.005 alpha exactly on both sides: kept
    assert dropped(lib, [below(thr_p), 1.0], [ap, ad])        # one ulp below on the primal side: dropped
    assert dropped(lib, [1.0, below(thr_d)], [ap, ad])        # the dual side alone failing
    assert not dropped(lib, [1.0, 1.0], [ap, ad])
    assert not dropped(lib, [NAN, NAN], [ap, ad])             # (comparisons with a NaN are false, as in the oracle)
    rng = np.random.default_rng(9)
    for _ in range(200):
        h, a = rng.uniform(0.0, 1.0, 2), rng.uniform(0.0, 1.0, 2)
        assert dropped(lib, h, a) == bool(h[0] < 1.005 * a[0] or h[1] < 1.005 * a[1])  # oracle/mpc.py:808


# ---- the decisions behind the corrector ---------------------------------------------------------------------------------------
def make_block(layout, *, info=0.0, pred=(1e-12, 3.0, 1.0), corr=(1e-12, 3.0, 1.0), alpha=(0.7, 0.8, 0.6, 0.9),
               gz_alpha=(0.5, 0.6, 0.4, 0.7), t_nrm=(1e-12, 3.0, 1.0), t_gz=(0.9, 0.95, 0.8, 0.85),
               t_tau=(0.88, 0.93, 0.78, 0.83)):
    blk = np.full(128, -3.0)  # (nothing else may be read)
    put = lambda name, v: blk.__setitem__(slice(layout[name][0], layout[name][0] + len(v)), v)
    put("INFO", [info])
    put("PRED_NRM", pred)
    put("CORR_NRM", corr)
    put("CORR_ALPHA", block8(*alpha))
    put("GZ_ALPHA", block8(*gz_alpha))
    put("TRIAL.nrm", t_nrm)
    put("TRIAL.alpha_gz", block8(*t_gz))
    put("TRIAL.alpha_tau", block8(*t_tau))
    return blk


def ref_decide(layout, blk, gondzio, max_ncorr, check, tol):
    """What the host does with the block (csrc/mpc.hip, body_fused), in the oracle's words: iteration_body's two
    solve_system calls, update_step's minima, and the first pass of gondzio_correction_direction's loop."""
    get = lambda name, n: blk[layout[name][0]:layout[name][0] + n]
    mins = lambda a8: (min(a8[0], a8[2]), min(a8[4], a8[6]))
    failed = lambda nrm: ref_failed(nrm, check, tol)[0]
    go = blk[layout["INFO"][0]] == 0.0 and not failed(get("PRED_NRM", 3)) and not failed(get("CORR_NRM", 3))
    ap, ad = mins(get("CORR_ALPHA", 8))
    restore = False
    if gondzio:
        alpha_p, alpha_d = mins(get("GZ_ALPHA", 8))         # :798
        go = go and not failed(get("TRIAL.nrm", 3))         # :806
        ha_p, ha_d = mins(get("TRIAL.alpha_gz", 8))         # :807
        if ha_p < 1.005 * alpha_p or ha_d < 1.005 * alpha_d:  # :808
            restore = go                                    # :809: the direction before it comes back
        else:
            ap, ad = mins(get("TRIAL.alpha_tau", 8))
            if max_ncorr > 1:
                go = False                                  # the loop goes round again: not the device's to do
    return [1.0 if go else 0.0, ap, ad, 1.0 if restore else 0.0]


def decide(lib, blk, gondzio, max_ncorr, check=False, tol=1e-8):
    out, po = arr(np.full(4, -9.0))
    lib.mpc_decide_c(arr(blk)[1], int(gondzio), max_ncorr, int(check), tol, po)
    return out


def test_decide(lib, layout):
    def both(expect, gondzio, max_ncorr, check=False, **kw):
        blk = make_block(layout, **kw)
        got = decide(lib, blk, gondzio, max_ncorr, check)
        assert same_bits(got, ref_decide(layout, blk, gondzio, max_ncorr, check, 1e-8)), (kw, got)
        assert same_bits(got, expect), (kw, got)

    both([1, 0.7, 0.6, 0], False, 0)                                   # no Gondzio: the corrector's minima
    both([1, 0.88, 0.78, 0], True, 1)                                  # the trial is kept and is the last: its step
    both([0, 0.88, 0.78, 0], True, 2)                                  # kept, another to run: the host takes over
    both([0, 0.88, 0.78, 0], True, 3)
    thr_p, thr_d = 1.005 * 0.5, 1.005 * 0.4
    below = lambda v: float(np.nextafter(v, 0.0))
    both([1, 0.88, 0.78, 0], True, 1, t_gz=(thr_p, 0.95, thr_d, 0.85))          # exactly 1.005 alpha: kept
    both([1, 0.7, 0.6, 1], True, 1, t_gz=(below(thr_p), 0.95, 0.8, 0.85))       # one ulp below: dropped, d restored
    both([1, 0.7, 0.6, 1], True, 1, t_gz=(0.9, 0.95, 0.8, below(thr_d)))        # the dual side alone
    both([1, 0.7, 0.6, 1], True, 3, t_gz=(0.9, 0.95, 0.8, below(thr_d)))        # dropped ends the loop whatever max_ncorr
    both([0, 0.7, 0.6, 0], False, 0, info=3.0)                                  # failed factorisation
    both([0, 0.88, 0.78, 0], True, 1, info=1.0)
    both([0, 0.7, 0.6, 0], True, 1, info=1.0, t_gz=(0.1, 0.95, 0.8, 0.85))      # ... nothing to restore: nothing is trusted
    both([0, 0.7, 0.6, 0], False, 0, pred=(NAN, 3.0, 1.0))                      # failed verdicts: predictor,
    both([0, 0.7, 0.6, 0], False, 0, corr=(NAN, 3.0, 1.0))                      #   corrector,
    both([1, 0.7, 0.6, 0], False, 0, check=False, corr=(4e-8, 3.0, 1.0))        #   (a ratio above the tolerance fails
    both([0, 0.7, 0.6, 0], False, 0, check=True, corr=(4e-8, 3.0, 1.0))         #   with check_residual only)
    both([1, 0.7, 0.6, 0], False, 0, check=True, corr=(2e-8, 3.0, 1.0))
    both([0, 0.88, 0.78, 0], True, 1, t_nrm=(NAN, 3.0, 1.0))                    #   trial
    both([0, 0.7, 0.6, 0], True, 1, t_nrm=(NAN, 3.0, 1.0), t_gz=(0.1, 0.95, 0.8, 0.85))
    both([1, 0.7, 0.6, 0], False, 0, t_nrm=(NAN, 3.0, 1.0))                     # (no Gondzio: the trial block is not read)
    both([1, 0.5, 0.25, 0], False, 0, alpha=(0.5, 0.5, 0.25, 0.25))             # ties in the minima
    both([1, 0.5, 0.25, 0], True, 1, t_tau=(0.5, 0.5, 0.25, 0.25))
    both([1, 0.88, 0.78, 0], True, 1, gz_alpha=(0.5, 0.5, 0.4, 0.4), t_gz=(thr_p, thr_p, thr_d, thr_d))
    rng = np.random.default_rng(11)
    for _ in range(300):
        u = lambda n: tuple(rng.uniform(0.0, 1.0, n))
        nrm = lambda: (10.0 ** rng.uniform(-10, -6), 10.0 ** rng.uniform(-2, 2), 1.0)
        blk = make_block(layout, info=float(rng.integers(0, 6) == 0), pred=nrm(), corr=nrm(), alpha=u(4), gz_alpha=u(4),
                         t_nrm=nrm(), t_gz=u(4), t_tau=u(4))
        for gondzio, max_ncorr in ((False, 0), (True, 1), (True, 2)):
            for check in (False, True):
                assert same_bits(decide(lib, blk, gondzio, max_ncorr, check), ref_decide(layout, blk, gondzio, max_ncorr, check, 1e-8))


# ---- the rules the batched engine calls too (csrc/batch_wg.inc), each against the oracle's own method on a stand-in solver --------
def bind_more(lib):
    ll = C.c_longlong
    lib.mpc_nanmax_c.argtypes, lib.mpc_nanmax_c.restype = [C.c_double, C.c_double], C.c_double
    lib.mpc_head_c.argtypes = [pd, C.c_double, C.c_double, C.c_double, ll, ll, pd]
    lib.mpc_queue_next_assembly_c.argtypes = [pd, C.c_double, ll, ll]
    lib.mpc_init_regularization_c.argtypes = [C.c_int, C.c_double, C.c_double, pd]
    lib.mpc_update_regularization_c.argtypes = [C.c_int] + [C.c_double] * 5 + [pd]
    lib.mpc_factorize_trials_c.argtypes = [C.c_int, pd]
    lib.mpc_blocking_c.argtypes = [pd, C.c_int]
    lib.mpc_mehrotra_step_c.argtypes = [pd, pd, pd, C.c_double, C.c_double, pd]
    lib.mpc_objective_c.argtypes, lib.mpc_objective_c.restype = [C.c_double] * 3, C.c_double
    lib.mpc_adjust_c.argtypes = [C.c_double, pd]
    lib.mpc_start_shifts_c.argtypes = [pd, pd, C.c_int, C.c_int, pd]
    return lib


@pytest.fixture(scope="module")
def rules(lib):
    return bind_more(lib)


@pytest.fixture(scope="module")
def O():
    from oracle import mpc
    return mpc


def same_or_nan(a, b):
    """same_bits, but a NaN equals any NaN: its sign and payload are the processor's, not the rule's."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return np.array_equal(np.isnan(a), np.isnan(b)) and same_bits(np.where(np.isnan(a), 0.0, a), np.where(np.isnan(b), 0.0, b))


class Stand:
    """A stand-in for oracle.mpc.MPCSolver that holds only what one method reads."""

    def __init__(self, **kw):
        self.__dict__.update(kw)


def test_status_codes_are_the_abis(lib, O):
    out = (C.c_int * 5)()
    lib.mpc_status_codes_c(out)
    assert list(out) == [0, O.SOLVE_SUCCEEDED, O.MAXIMUM_ITERATIONS_EXCEEDED, -3, -1] == [0, 1, 6, -3, -1]


# -- iteration_head (oracle/mpc.py:821-833)
def ref_head(O, nrm, norm_b, norm_c, tol, k, max_iter):
    s = Stand(kkt=Stand(jtprod=lambda y: np.zeros(1)), y=None, jacl=np.zeros(1), c=np.array([nrm[0]]), f=np.array([nrm[1]]),
              zl=np.zeros(1), zu=np.zeros(1), norm_b=norm_b, norm_c=norm_c, get_optimality_gap=lambda: f64(nrm[2]),
              record=lambda: None, opt=Stand(tol=tol, max_iter=max_iter), k=k)
    with np.errstate(all="ignore"):
        st = O.MPCSolver.iteration_head(s)
    return [s.inf_pr, s.inf_du, s.inf_compl], 0 if st is None else st


def head(rules, nrm, norm_b, norm_c, tol, k, max_iter):
    out, po = arr(np.zeros(3))
    st = rules.mpc_head_c(arr(np.abs(nrm))[1], norm_b, norm_c, tol, k, max_iter, po)
    return list(out), st


def test_head_is_bitwise_the_oracles(rules, O):
    rng = np.random.default_rng(21)
    for _ in range(400):
        nrm = 10.0 ** rng.uniform(-10, -6, 3)
        norm_b, norm_c = 10.0 ** rng.uniform(-2, 2, 2)  # both sides of max(1, .)
        k, max_iter = int(rng.integers(0, 4)), int(rng.integers(0, 4))
        got, ref = head(rules, nrm, norm_b, norm_c, 1e-8, k, max_iter), ref_head(O, nrm, norm_b, norm_c, 1e-8, k, max_iter)
        assert same_bits(got[0], ref[0]) and got[1] == ref[1]


def test_head_on_both_sides_of_its_branches(rules, O):
    tol = 1e-8
    above = float(np.nextafter(tol, 1.0))
    for nrm, k, max_iter, want in (([tol, tol, tol], 0, 10, 1), ([above, tol, tol], 0, 10, 0), ([tol, above, tol], 0, 10, 0),
                                   ([tol, tol, above], 0, 10, 0), ([above, 0, 0], 10, 10, 6), ([above, 0, 0], 9, 10, 0),
                                   ([tol, tol, tol], 10, 10, 1), ([0, 0, 0], 0, 0, 1), ([1, 1, 1], 0, 0, 6)):
        got = head(rules, nrm, 1.0, 1.0, tol, k, max_iter)
        assert got[1] == want == ref_head(O, nrm, 1.0, 1.0, tol, k, max_iter)[1], (nrm, k, max_iter)
    # the scale is max(1, norm): norm_b scales the primal residual only, norm_c the other two
    assert head(rules, [8.0, 8.0, 8.0], 4.0, 0.5, tol, 0, 9) == ([2.0, 8.0, 8.0], 0)
    assert head(rules, [8.0, 8.0, 8.0], 0.5, 4.0, tol, 0, 9) == ([8.0, 2.0, 2.0], 0)


def test_head_with_non_finite_operands(rules, O):
    """max(inf_pr, inf_du, inf_compl) folds from the left with `>`: a NaN in the first place stays (not solved), one in a
    later place is passed over -- Python's and std::max's order, which both native drivers now take."""
    tol = 1e-8
    table = [([NAN, 0, 0], 0), ([0, NAN, 0], 1), ([0, 0, NAN], 1), ([0, NAN, 1], 0), ([1, NAN, 0], 0), ([NAN, NAN, NAN], 0),
             ([INF, 0, 0], 0), ([0, INF, 0], 0), ([0, 0, INF], 0), ([NAN, INF, 0], 0)]
    for nrm, want in table:
        got, ref = head(rules, nrm, 1.0, 1.0, tol, 0, 10), ref_head(O, nrm, 1.0, 1.0, tol, 0, 10)
        assert same_bits(got[0], ref[0]) and got[1] == ref[1] == want, (nrm, got, ref)
        assert head(rules, nrm, 1.0, 1.0, tol, 10, 10)[1] == ref_head(O, nrm, 1.0, 1.0, tol, 10, 10)[1] == (want or 6)
    for nb, nc in ((NAN, 1.0), (1.0, NAN), (INF, INF), (NAN, NAN)):  # max(1.0, NaN) is 1.0; x / inf is 0
        got, ref = head(rules, [3.0, 3.0, 3.0], nb, nc, tol, 0, 10), ref_head(O, [3.0, 3.0, 3.0], nb, nc, tol, 0, 10)
        assert same_bits(got[0], ref[0]) and got[1] == ref[1], (nb, nc)
    assert head(rules, [INF, 1.0, 1.0], INF, 1.0, tol, 0, 10)[1] == 0  # inf / inf: NaN first, not solved
    # the optimality gap of the reduction kernels keeps a NaN on either side (np.max does, over the whole list)
    nm = rules.mpc_nanmax_c
    assert nm(1.0, 2.0) == 2.0 and nm(2.0, 1.0) == 2.0 and nm(INF, 1.0) == INF and nm(-0.0, 0.0) in (0.0, -0.0)
    assert math.isnan(nm(NAN, 1.0)) and math.isnan(nm(1.0, NAN)) and math.isnan(nm(NAN, INF))
    assert all(nm(a, b) == np.max([a, b]) for a, b in np.random.default_rng(1).uniform(0, 1, (50, 2)))


def test_next_assembly_is_queued_unless_the_loop_is_about_to_end(rules):
    q = lambda inf3, k, max_iter: bool(rules.mpc_queue_next_assembly_c(arr(inf3)[1], 1e-8, k, max_iter))
    edge = 100.0 * 1e-8
    assert not q([edge, 0, 0], 0, 10) and q([float(np.nextafter(edge, 1.0)), 0, 0], 0, 10)
    assert q([0, 1.0, 0], 0, 10) and q([0, 0, 1.0], 0, 10) and not q([0, 0, 0], 0, 10)
    assert q([1.0, 0, 0], 8, 10) and not q([1.0, 0, 0], 9, 10)  # the last pass allowed queues nothing
    assert q([NAN, 0, 0], 0, 10) and not q([0, NAN, 0], 0, 10) and q([0, NAN, 1.0], 0, 10) and q([INF, 0, 0], 0, 10)


# -- init_regularization, update_regularization (oracle/mpc.py:641-655)
def oracle_reg(O, mode, dp, dd, dmin):
    return (O.NoRegularization(), O.FixedRegularization(dp, dd), O.AdaptiveRegularization(dp, dd, dmin))[mode]


def test_regularization_is_bitwise_the_oracles(rules, O):
    rng = np.random.default_rng(23)
    cases = [(10.0 ** rng.uniform(-12, -4), -10.0 ** rng.uniform(-12, -4), 10.0 ** rng.uniform(-12, -6)) for _ in range(60)]
    # either side of delta_min: the shrinking pair stops at +-delta_min, from exactly 10 delta_min and one ulp around it
    cases += [(1e-8, -1e-8, 1e-9), (float(np.nextafter(1e-8, 1)), -float(np.nextafter(1e-8, 1)), 1e-9),
              (float(np.nextafter(1e-8, 0)), -float(np.nextafter(1e-8, 0)), 1e-9), (1e-9, -1e-9, 1e-9), (1e-12, -1e-12, 1e-9),
              (0.0, 0.0, 0.0), (1e-8, 0.0, 1e-9), (INF, -INF, 1e-9), (NAN, NAN, 1e-9), (1e-8, -1e-8, NAN), (NAN, -1e-8, INF)]
    for dp, dd, dmin in cases:
        for mode in (0, 1, 2):
            reg = oracle_reg(O, mode, dp, dd, dmin)
            s = Stand(opt=Stand(regularization=reg))
            out, po = arr(np.zeros(4))
            rules.mpc_init_regularization_c(mode, dp, dd, po)
            O.MPCSolver.init_regularization(s)
            assert same_bits(out, [s.del_w, s.del_c, dp, dd]), (mode, dp, dd)
            assert s.del_w == 1.0 and (mode != 0 or s.del_c == 0.0)
            run = out[2:].copy()
            for _ in range(5):  # the running pair over five passes
                rules.mpc_update_regularization_c(mode, dp, dd, dmin, run[0], run[1], po)
                O.MPCSolver.update_regularization(s)
                want_run = [reg.delta_p, reg.delta_d] if mode == 2 else run
                assert same_bits(out, [s.del_w, s.del_c] + list(want_run)), (mode, dp, dd, dmin, out)
                run = out[2:].copy()
    out, po = arr(np.zeros(4))
    rules.mpc_update_regularization_c(2, 1e-8, -1e-8, 1e-9, 1e-8, -1e-8, po)
    assert same_bits(out, [1e-8 / 10.0, -1e-8 / 10.0, 1e-8 / 10.0, -1e-8 / 10.0])
    rules.mpc_update_regularization_c(2, 1e-8, -1e-8, 1e-9, 5e-9, -5e-9, po)
    assert same_bits(out, [1e-9, -1e-9, 1e-9, -1e-9])
    rules.mpc_update_regularization_c(2, 1e-8, -1e-8, 1e-9, NAN, NAN, po)  # max(NaN, x), min(NaN, x): the NaN stays
    assert np.isnan(out).all()
    rules.mpc_update_regularization_c(2, 1e-8, -1e-8, NAN, 1e-8, -1e-8, po)  # max(x, NaN), min(x, NaN): x
    assert same_bits(out, [1e-9, -1e-9, 1e-9, -1e-9])


# -- factorize_regularized_system (oracle/mpc.py:663-670)
def test_retry_is_bitwise_the_oracles(rules, O):
    rng = np.random.default_rng(27)
    dels = [tuple(rng.uniform(-1, 1, 2) * 10.0 ** rng.uniform(-12, 0)) for _ in range(40)]
    dels += [(1e-8, -1e-8), (0.0, -0.0), (1e300, -1e300), (INF, -INF), (NAN, 1.0), (1.0, NAN)]
    for dw, dc in dels:
        for failures in range(5):  # 0 .. 2 failed trials go on; from 3 the third is the last all the same
            calls = []
            kkt = Stand(build_and_factorize=lambda: calls.append(1), is_factorized=lambda: len(calls) > failures)
            s = Stand(del_w=f64(dw), del_c=f64(dc), kkt=kkt, set_aug_diagonal_reg=lambda: None)
            with np.errstate(all="ignore"):
                O.MPCSolver.factorize_regularized_system(s)
            d2, p2 = arr([dw, dc])
            n = rules.mpc_factorize_trials_c(failures, p2)
            assert n == len(calls) == min(failures + 1, 3) and same_bits(d2, [s.del_w, s.del_c]), (dw, dc, failures)
    d2, p2 = arr([1e-8, -1e-8])
    assert rules.mpc_factorize_trials_c(1, p2) == 2 and same_bits(d2, [1e-8 * 100.0, -1e-8 * 100.0])


# -- update_step, the MehrotraAdaptiveStep branch (oracle/mpc.py:616-639)
def ref_mehrotra(O, a4, ib, lb, ub, mean, gamma_f):
    """lb, ub: dicts of the arrays the branch reads over the lower / the upper bounds (x, b, z, dx, dz)."""
    s = Stand(opt=Stand(step_rule=O.MehrotraAdaptiveStep(gamma_f)), d=Stand(zl=lb["dz"], zu=ub["dz"]),
              get_alpha_max_primal=lambda tau: (a4[0], a4[1], ib[0], ib[1]),
              get_alpha_max_dual=lambda tau: (a4[2], a4[3], ib[2], ib[3]),
              get_affine_complementarity_measure=lambda ap, ad: f64(mean),
              zl_r=lb["z"], x_lr=lb["x"], xl_r=lb["b"], dx_lr=lb["dx"], zu_r=ub["z"], x_ur=ub["x"], xu_r=ub["b"], dx_ur=ub["dx"])
    with np.errstate(all="ignore"):
        O.MPCSolver.update_step(s)
    return [s.alpha_p, s.alpha_d]


def mehrotra(rules, a4, ib, lb, ub, mean, gamma_f):
    """The drivers' part: the rows at the blocking indices mpc_blocking names, then the rule."""
    rows = np.full((2, 5), -77.0)  # (a row the rule must not read where its step is free)
    for dual in (0, 1):
        k = rules.mpc_blocking_c(arr(a4)[1], dual)
        assert k in (-1, 2 * dual, 2 * dual + 1)
        if k >= 0:
            t = ub if k & 1 else lb
            rows[dual] = [t[key][ib[k]] for key in ("x", "b", "z", "dx", "dz")]
    out, po = arr(np.zeros(2))
    rules.mpc_mehrotra_step_c(arr(a4)[1], arr(rows[0])[1], arr(rows[1])[1], mean, gamma_f, po)
    return list(out)


def bound_arrays(rng, n, upper):
    x, gap = rng.uniform(-2, 2, n), 10.0 ** rng.uniform(-6, 0, n)
    return dict(x=x, b=x + gap if upper else x - gap, z=10.0 ** rng.uniform(-6, 1, n), dx=rng.uniform(-1, 1, n),
                dz=rng.uniform(-1, 1, n))


def test_mehrotra_step_is_bitwise_the_oracles(rules, O):
    rng = np.random.default_rng(29)
    for it in range(600):
        lb, ub = bound_arrays(rng, 5, False), bound_arrays(rng, 5, True)
        a4 = [float(v) if rng.random() < 0.7 else 1.0 for v in rng.uniform(0, 1, 4)]  # 1.0: nothing blocks on that side
        if it % 7 == 0:
            a4[1], a4[3] = a4[0], a4[2]  # ties go to the lower bound
        ib = [int(rng.integers(0, 5)) if a < 1.0 else -1 for a in a4]
        mean, gamma_f = 10.0 ** rng.uniform(-9, 1), float(rng.choice([0.99, 0.9, 0.5]))
        assert same_bits(mehrotra(rules, a4, ib, lb, ub, mean, gamma_f), ref_mehrotra(O, a4, ib, lb, ub, mean, gamma_f)), (a4, ib)


def test_mehrotra_step_on_both_sides_of_its_branches(rules, O):
    one = lambda x, b, z, dx, dz: dict(x=np.array([x]), b=np.array([b]), z=np.array([z]), dx=np.array([dx]), dz=np.array([dz]))
    lb, ub = one(1.0, 0.0, 2.0, -4.0, -3.0), one(1.0, 3.0, 2.0, 5.0, -6.0)
    below = float(np.nextafter(1.0, 0.0))
    blocking = lambda a4, dual: rules.mpc_blocking_c(arr(a4)[1], dual)
    assert [blocking([1.0, 1.0, 1.0, 1.0], d) for d in (0, 1)] == [-1, -1]              # nothing below 1: both steps free
    assert [blocking([below, 1.0, 1.0, below], d) for d in (0, 1)] == [0, 3]            # one ulp below: lower / upper
    assert [blocking([0.5, 0.5, 0.25, 0.25], d) for d in (0, 1)] == [0, 2]              # a tie is the lower bound's
    assert [blocking([0.5, float(np.nextafter(0.5, 0)), 0.25, float(np.nextafter(0.25, 0))], d) for d in (0, 1)] == [1, 3]
    assert [blocking([NAN, 0.5, 0.5, NAN], d) for d in (0, 1)] == [-1, 3]  # min(NaN, x) is NaN: free; min(x, NaN) is x, NaN <= x false
    for a4, ib in (([1.0, 1.0, 1.0, 1.0], [-1] * 4), ([0.5, 1.0, 1.0, 1.0], [0, -1, -1, -1]), ([1.0, 0.5, 1.0, 1.0], [-1, 0, -1, -1]),
                   ([1.0, 1.0, 0.5, 1.0], [-1, -1, 0, -1]), ([1.0, 1.0, 1.0, 0.5], [-1, -1, -1, 0]), ([0.5, 0.5, 0.25, 0.25], [0] * 4),
                   ([0.25, 0.5, 0.5, 0.25], [0] * 4), ([below, 1.0, below, 1.0], [0, -1, 0, -1])):
        for mean in (0.0, 1e-3, 10.0):  # (a large mean: the blocking formula falls below gamma_f max_alpha, the floor wins)
            got = mehrotra(rules, a4, ib, lb, ub, mean, 0.99)
            assert same_bits(got, ref_mehrotra(O, a4, ib, lb, ub, mean, 0.99)), (a4, mean, got)
    # figures: gamma_a = 1 / (1 - 0.5) = 2, mu_full = 0.8 / 2 = 0.4; primal at the lower bound: tmp = 0.4 / (2 + 0.5 * -3) = 0.8,
    # alpha_p = (1 - 0 - 0.8) / 4 = 0.05 < 0.5 * 0.25: the floor; dual at the upper: tmp = 0.4 / (3 - 1 - 0.25 * 5) = 0.5333..,
    # alpha_d = -(2 - tmp) / -6
    got = mehrotra(rules, [0.25, 1.0, 1.0, 0.5], [0, -1, -1, 0], lb, ub, 0.8, 0.5)
    tmp = 0.4 / (3.0 - 1.0 - 0.25 * 5.0)
    assert same_bits(got, [0.125, max(-(2.0 - tmp) / -6.0, 0.25)]) and got[1] == 0.25
    got = mehrotra(rules, [0.25, 1.0, 1.0, 0.5], [0, -1, -1, 0], lb, ub, 0.08, 0.5)
    tmp = 0.04 / (3.0 - 1.0 - 0.25 * 5.0)  # a tenth of the mean: both formulas lie above their floors
    assert same_bits(got, [(1.0 - 0.04 / (2.0 + 0.5 * -3.0)) / 4.0, -(2.0 - tmp) / -6.0]) and got[0] > 0.125 and got[1] > 0.25


def test_mehrotra_step_with_non_finite_operands(rules, O):
    """max(alpha, gamma_f max_alpha) keeps a NaN alpha (its first operand), as the oracle and the host driver always did."""
    one = lambda x, b, z, dx, dz: dict(x=np.array([x]), b=np.array([b]), z=np.array([z]), dx=np.array([dx]), dz=np.array([dz]))
    a4, ib = [0.5, 1.0, 0.25, 1.0], [0, -1, 0, -1]
    ub = one(1.0, 3.0, 2.0, 5.0, -6.0)
    for pos in range(5):
        for bad in (NAN, INF, -INF, 0.0):
            v = [1.0, 0.0, 2.0, -4.0, -3.0]
            v[pos] = bad
            for mean in (1e-3, NAN, INF, 0.0):
                got = mehrotra(rules, a4, ib, one(*v), ub, mean, 0.99)
                assert same_or_nan(got, ref_mehrotra(O, a4, ib, one(*v), ub, mean, 0.99)), (pos, bad, mean, got)
    got = mehrotra(rules, a4, ib, one(1.0, 0.0, 0.0, 0.0, 0.0), ub, 0.0, 0.99)  # 0 / 0 in both formulas: no floor under a NaN
    assert same_or_nan(got, ref_mehrotra(O, a4, ib, one(1.0, 0.0, 0.0, 0.0, 0.0), ub, 0.0, 0.99)) and np.isnan(got).all()
    got = mehrotra(rules, a4, ib, one(1.0, 0.0, 2.0, 0.0, 0.0), ub, 0.0, 0.99)  # x / -0 and -x / 0: -inf, the floors
    assert same_bits(got, [0.99 * 0.5, 0.99 * 0.25])
    got = mehrotra(rules, a4, ib, one(NAN, 0.0, 2.0, -4.0, -3.0), ub, 1e-3, 0.99)
    assert math.isnan(got[0]) and math.isnan(got[1])
    for gamma_f in (NAN, 0.0):  # gamma_a = NaN, or 1: no floor (gamma_f = 1 divides by zero, which the oracle refuses)
        got = mehrotra(rules, a4, ib, one(1.0, 0.0, 2.0, -4.0, -3.0), ub, 1e-3, gamma_f)
        assert same_or_nan(got, ref_mehrotra(O, a4, ib, one(1.0, 0.0, 2.0, -4.0, -3.0), ub, 1e-3, gamma_f))
    assert same_or_nan(mehrotra(rules, [1.0] * 4, [-1] * 4, ub, ub, NAN, 0.99), [1.0, 1.0])  # no bound blocks: the mean is not read


# -- the objective and adjust_boundary (oracle/mpc.py:189-196)
def test_objective_and_adjust_boundary_constants(rules, O):
    rng = np.random.default_rng(31)
    for c0, lin, quad in rng.uniform(-1, 1, (100, 3)) * 10.0 ** rng.uniform(-3, 3, (100, 1)):
        assert same_bits(rules.mpc_objective_c(c0, lin, quad), f64(c0) + f64(lin) + 0.5 * f64(quad))
    for t in ((NAN, 1, 1), (1, NAN, 1), (1, 1, NAN), (INF, -INF, 1), (1, INF, -INF), (INF, 1, 1)):
        with np.errstate(invalid="ignore"):
            assert same_bits(rules.mpc_objective_c(*map(float, t)), f64(t[0]) + f64(t[1]) + 0.5 * f64(t[2]))
    out, po = arr(np.zeros(2))
    for mu in list(10.0 ** rng.uniform(-11, 0, 50)) + [0.0, 1e-11, 0.1, INF, NAN]:
        rules.mpc_adjust_c(float(mu), po)
        assert same_bits(out, [O.EPS * f64(mu), O.EPS ** 0.75])
    # ... and they are the two the oracle's adjust_boundary acts on: a bound at distance c1 stays, one ulp nearer it moves by c2 max(1, |x|)
    mu = 0.1
    rules.mpc_adjust_c(mu, po)
    c1, c2 = out
    for x in (0.25, -7.5):
        # (bounds an exact power-of-two multiple of c1 away, so that x - xl is that distance to the bit)
        xl, xu = np.array([x - 2 * c1 * 2.0 ** 52, x - c1 * 2.0 ** 51]), np.array([x + 2 * c1 * 2.0 ** 52, x + c1 * 2.0 ** 51])
        xs = np.array([x, x])
        want_l, want_u = xl.copy(), xu.copy()
        for j in range(2):
            if xs[j] - xl[j] < c1:
                want_l[j] = xl[j] - c2 * max(1.0, abs(xs[j]))
            if xu[j] - xs[j] < c1:
                want_u[j] = xu[j] + c2 * max(1.0, abs(xs[j]))
        O.adjust_boundary(xs, xl, xu, np.arange(2), np.arange(2), mu)
        assert same_bits(xl, want_l) and same_bits(xu, want_u)
    xs, xl, xu = np.array([1.0, 1.0, 4.0]), np.array([1.0 - 1e-3, 1.0, 4.0]), np.array([2.0, 1.0, 4.0])
    O.adjust_boundary(xs, xl, xu, np.arange(3), np.arange(3), mu)
    assert same_bits(xl, [1.0 - 1e-3, 1.0 - c2, 4.0 - c2 * 4.0]) and same_bits(xu, [2.0, 1.0 + c2, 4.0 + c2 * 4.0])


# -- init_starting_point's two shifts (oracle/mpc.py:711-726)
def ref_start_shifts(x, l, u, zl, zu, ilb, iub):
    """oracle/mpc.py:711-726, line for line, on copies; returns the four shifts and what the rule is given: the four minima
    before the first shift and the eight sums behind it (csrc/vec_kernels.inc: sp_mins_kernel, sp_sums_kernel)."""
    x, zl, zu = x.copy(), zl.copy(), zu.copy()
    mn = [np.min(x[ilb] - l[ilb], initial=0.0), np.min(u[iub] - x[iub], initial=0.0), np.min(zl[ilb], initial=0.0),
          np.min(zu[iub], initial=0.0)]
    delta_x = max(0.0, -1.5 * np.min(x[ilb] - l[ilb], initial=0.0), -1.5 * np.min(u[iub] - x[iub], initial=0.0))
    delta_s = max(0.0, -1.5 * np.min(zl[ilb], initial=0.0), -1.5 * np.min(zu[iub], initial=0.0))
    x[ilb] = x[ilb] + delta_x
    x[iub] = x[iub] - delta_x
    zl[ilb] += 1.0 + delta_s
    zu[iub] += 1.0 + delta_s
    sm = [x[ilb] @ zl[ilb], l[ilb] @ zl[ilb], u[iub] @ zu[iub], x[iub] @ zu[iub], np.sum(zl[ilb]), np.sum(zu[iub]),
          np.sum(x[ilb] - l[ilb]), np.sum(u[iub] - x[iub])]
    mu = 0.0
    if len(ilb) > 0:
        mu += x[ilb] @ zl[ilb] - l[ilb] @ zl[ilb]
    if len(iub) > 0:
        mu += u[iub] @ zu[iub] - x[iub] @ zu[iub]
    with np.errstate(invalid="ignore", divide="ignore"):
        delta_x2 = np.float64(mu) / (2 * (np.sum(zl[ilb]) + np.sum(zu[iub])))
        delta_s2 = np.float64(mu) / (2 * (np.sum(x[ilb] - l[ilb]) + np.sum(u[iub] - x[iub])))
    return [delta_x, 1.0 + delta_s, delta_x2, delta_s2], mn, sm


def start_shifts(rules, mn, sm, has_lb, has_ub):
    out, po = arr(np.zeros(4))
    rules.mpc_start_shifts_c(arr(mn)[1], arr(sm)[1], int(has_lb), int(has_ub), po)
    return out


def test_start_shifts_are_bitwise_the_oracles(rules):
    rng = np.random.default_rng(33)
    for it in range(300):
        n = 9
        ilb = np.flatnonzero(rng.random(n) < (0.0 if it % 10 == 0 else 0.7))  # every tenth: no lower bound / no upper bound / none
        iub = np.flatnonzero(rng.random(n) < (0.0 if it % 10 in (1, 0) and it % 20 < 10 else 0.7))
        x = rng.uniform(-2, 2, n)
        shift = rng.uniform(-0.5, 1.5, n) if it % 3 else rng.uniform(0.1, 1.5, n)  # x outside its bounds or all inside
        l, u = x - shift, x + rng.uniform(-0.5, 1.5, n) if it % 3 else x + rng.uniform(0.1, 1.5, n)
        zl = rng.uniform(-1, 1, n) if it % 2 else rng.uniform(0.1, 1, n)
        zu = rng.uniform(-1, 1, n) if it % 2 else rng.uniform(0.1, 1, n)
        want, mn, sm = ref_start_shifts(x, l, u, zl, zu, ilb, iub)
        assert same_bits(start_shifts(rules, mn, sm, len(ilb) > 0, len(iub) > 0), want), (it, mn, sm)


def test_start_shifts_on_both_sides_of_their_branches(rules):
    sm = [3.0, 1.0, 7.0, 2.0, 0.5, 1.5, 0.25, 0.75]
    ss = lambda mn, lb=True, ub=True, s=sm: start_shifts(rules, mn, s, lb, ub)
    assert same_bits(ss([0.0, 0.0, 0.0, 0.0])[:2], [0.0, 1.0])                   # all inside: nothing moves (max(0.0, -0.0, -0.0) is 0.0)
    assert same_bits(ss([-2.0, 0.0, 0.0, -4.0])[:2], [3.0, 7.0])                 # 1.5 times the worst violation, on either side
    assert same_bits(ss([0.0, -2.0, -4.0, 0.0])[:2], [3.0, 7.0])
    assert same_bits(ss([-2.0, -3.0, -1.0, -0.5])[:2], [4.5, 2.5])
    assert same_bits(ss([-5e-324, 0.0, 0.0, 0.0])[:2], [-1.5 * -5e-324, 1.0])
    # the second pair: mu over twice the sums, each side's part only where that side has bounds
    assert same_bits(ss([0] * 4)[2:], [7.0 / (2 * 2.0), 7.0 / (2 * 1.0)])
    assert same_bits(ss([0] * 4, ub=False)[2:], [2.0 / (2 * 2.0), 2.0 / (2 * 1.0)])
    assert same_bits(ss([0] * 4, lb=False)[2:], [5.0 / (2 * 2.0), 5.0 / (2 * 1.0)])
    got = ss([0] * 4, lb=False, ub=False, s=[0.0] * 8)                           # no bound at all: 0 / 0
    assert same_bits(got[:2], [0.0, 1.0]) and np.isnan(got[2:]).all()
    # non-finite operands: max(0.0, a, b) passes a NaN over in either place; an infinite violation is an infinite shift
    py = lambda mn: [max(0.0, -1.5 * f64(mn[0]), -1.5 * f64(mn[1])), 1.0 + max(0.0, -1.5 * f64(mn[2]), -1.5 * f64(mn[3]))]
    for mn in ([NAN, -2.0, 0, 0], [-2.0, NAN, 0, 0], [NAN, NAN, NAN, NAN], [0, 0, NAN, -2.0], [0, 0, -2.0, NAN], [-INF, 0, 0, -INF],
               [NAN, 0.0, 0.0, NAN]):
        assert same_bits(ss(mn)[:2], py(mn)), mn
    assert same_bits(ss([NAN, -2.0, -2.0, NAN])[:2], [3.0, 4.0]) and same_bits(ss([NAN] * 4)[:2], [0.0, 1.0])
    for k in range(8):
        for bad in (NAN, INF, -INF):
            s2 = list(sm)
            s2[k] = bad
            with np.errstate(invalid="ignore", divide="ignore"):
                mu = (f64(s2[0]) - f64(s2[1])) + (f64(s2[2]) - f64(s2[3]))
                want = [mu / (2 * (f64(s2[4]) + f64(s2[5]))), mu / (2 * (f64(s2[6]) + f64(s2[7])))]
            assert same_bits(ss([0] * 4, s=s2)[2:], want), (k, bad)
