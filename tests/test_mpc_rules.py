"""The result-block layout and the scalar rules of the fused iteration (madqp_jl_amd/csrc/mpc_rules.inc, compiled for the
CPU by tests/csrc): the functions the native driver (csrc/mpc.hip) and its one-thread kernels (csrc/vec_kernels.hip) both
call, held to the arithmetic of oracle/mpc.py -- update_barrier, solve_system's verdict, get_fraction_to_boundary_step and
gondzio_correction_direction (oracle/mpc.py:795-812) -- bit for bit, and to explicit figures on both sides of every
constant.  No GPU."""
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
