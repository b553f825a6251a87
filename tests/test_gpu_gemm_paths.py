"""GPU: every launch form of the fp64 MFMA product (csrc/gemm_f64.hip: madqp_gemm_tn and its kernels) against a plain
reference of the same operation, through the test seam madqp_debug_gemm_tn.

The dispatcher picks among about ten launch forms from the tile count, K, the resident workgroups and a cost model;
every one of them is "the same numbers by another schedule".  Each case here
  * holds every written entry to the bound DERIVED in tests/gemm_paths.py (2 (K + 4) u S against float64 numpy,
    (K + 4) u S against an extended-precision reference on a sample; no tolerance is tuned from what the kernel gives),
  * checks that nothing else was written (C is NaN outside what the call may write, bits compared),
  * asserts from the dispatcher's own report that the launch form under test really ran -- a later change of the cost
    model fails the case by name instead of silently ending its coverage.  Exact figures hold for 512 resident workgroups
    (256 CUs); on another device the qualitative form is asserted.
Bitwise claims the source makes are asserted as such: split forms give the same bytes on every run; the persistent, the
segmented and the un-remapped (MADQP_GEMM_XCD=0) launches give the bytes of the plain launch.  The interior LDS-DMA loop
and the register-staged loop (gemm_core.inc) feed the MFMAs in the same k order -- stage by stage, k-steps kk = 0..3 of
rows kk * 4 + (lane >> 4) in both -- so for K % 16 == 0 their results are asserted bitwise equal, too."""
import copy
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import gemm_paths as G
from gemm_paths import Problem, check, run, same_bits, seam

pytestmark = pytest.mark.gpu

ERR_ARG = -1


def expect(info, label, **want):
    """The launch form under test must have run.  Callables are qualitative rules that hold on every device; plain
    values are the figures for 512 resident workgroups."""
    for k, v in want.items():
        if callable(v):
            assert v(info[k]), f"{label}: the dispatcher no longer takes this path ({k} = {info[k]}): {info}"
        elif info["gemm_slots"] == 512:
            assert info[k] == v, f"{label}: the dispatcher no longer takes this path ({k} = {info[k]}, expected {v}): {info}"


ge2 = lambda v: v >= 2
pos = lambda v: v > 0
one = lambda v: v == 1
zero = lambda v: v == 0

# (label, M, N, K, lower, options of the problem, expected dispatch, run twice for identical bytes)
PATHS = [
    ("split2", 300, 300, 600, 1, {}, dict(ntiles=6, ksplit=2, kchunk=304, tail_tiles=0), True),
    ("split14", 1000, 1000, 5000, 1, {}, dict(ntiles=36, ksplit=14, kchunk=368, tail_tiles=0), True),
    ("split5_general", 2300, 640, 1660, 0, dict(alpha=-1.0, cin="alias", dvec=False),
     dict(ntiles=90, ksplit=5, kchunk=336, tail_tiles=0), True),
    ("split2_upper_edge", 2800, 2800, 520, 1, {}, dict(ntiles=253, ksplit=2, kchunk=272), True),
    ("tail308x3", 5000, 5000, 2000, 1, {}, dict(ntiles=820, ksplit=1, tail_tiles=308, tail_split=3, kchunk=672), True),
    ("tail308x3_k2016", 5000, 5000, 2016, 1, {}, dict(ntiles=820, ksplit=1, tail_tiles=308, tail_split=3, kchunk=672), True),
    ("tail16x4", 4000, 4000, 1024, 1, {}, dict(ntiles=528, ksplit=1, tail_tiles=16, tail_split=4, kchunk=256), True),
    ("tail4x5", 7000, 7000, 1500, 1, {}, dict(ntiles=1540, ksplit=1, tail_tiles=4, tail_split=5, kchunk=304), True),
    ("few_rounds_x3", 5000, 5000, 8192, 1, {}, dict(ntiles=820, ksplit=3, kchunk=2736, tail_tiles=0), True),
    ("few_rounds_x2", 6000, 6000, 6000, 1, {}, dict(ntiles=1128, ksplit=2, kchunk=3008, tail_tiles=0), True),
    ("whole_staged", 3000, 3000, 4100, 1, {}, dict(ntiles=300, ksplit=1, tail_tiles=0, segments=1), False),
    ("whole_staged_general", 5000, 1280, 3720, 0, {}, dict(ntiles=400, ksplit=1, tail_tiles=0, segments=1), False),
]
QUALITATIVE = {
    "split": dict(ksplit=ge2, tail_tiles=zero, segments=one, persistent_workgroups=zero),
    "tail": dict(ksplit=one, tail_tiles=pos, tail_split=ge2, persistent_workgroups=zero),
    "few_rounds": dict(ksplit=ge2, tail_tiles=zero, persistent_workgroups=zero),
    "whole": dict(ksplit=one, tail_tiles=zero, persistent_workgroups=zero),
}


@pytest.mark.parametrize("label,M,N,K,lower,opts,want,twice", PATHS, ids=[c[0] for c in PATHS])
def test_launch_form(hip, label, M, N, K, lower, opts, want, twice):
    """The path table: split-K of few tiles, the cost-model split of a few rounds of long tiles, the tail split and the
    two unsplit controls (K not a multiple of 16: the register-staged loop on every tile).  All CPU references are full
    float64 products (a few seconds at 5000 x 5000 x 8192) plus the extended-precision sample."""
    o = dict(cin="sep", dvec=True)
    o.update(opts)
    p = Problem(M * 31 + N * 7 + K, M, N, K, lower=lower, **o)
    rc, info, out, prior = run(hip, p)
    assert rc == 0, hip.lib.madqp_last_error(hip.ctx)
    expect(info, label, **next(v for k, v in QUALITATIVE.items() if label.startswith(k)))
    expect(info, label, **want)
    check(p, out, prior, info, label)
    if twice:  # "same result on every run": chunks are summed in chunk order, not in order of arrival
        rc, info2, out2, _ = run(hip, p)
        assert rc == 0 and info2 == info
        assert same_bits(out, out2), f"{label}: two runs of the same split launch differ"


def test_persistent_launch_gives_the_bytes_of_the_plain_launch(hip):
    """gemm_tn_f64_persistent_kernel (per-XCD ticket counters, csrc/dist.hip's capped launches): 384 and 8 workgroups
    work off 820 tiles.  "Which workgroup computes a tile does not enter the result": bytes equal to the plain launch.
    Two capped calls in one process -- the tickets must be zeroed before each."""
    p = Problem(77, 5000, 5000, 512, lower=1, cin="sep", dvec=True)
    rc, info, plain, prior = run(hip, p)
    assert rc == 0
    expect(info, "plain", ntiles=820, ksplit=one, tail_tiles=zero, persistent_workgroups=zero, segments=one)
    check(p, plain, prior, info, "persistent/plain")
    for cap, wgs in ((128, 384), (500, 8)):
        rc, info, out, prior = run(hip, p, cap_slots=cap)
        assert rc == 0
        label = f"persistent/cap{cap}"
        expect(info, label, persistent_workgroups=pos, segments=zero, ksplit=one, tail_tiles=zero)
        expect(info, label, persistent_workgroups=wgs)
        check(p, out, prior, info, label, full=False)
        assert same_bits(out, plain), f"{label}: differs from the plain launch"
    rc, info, out, _ = run(hip, p)  # the cap does not outlive the call
    assert rc == 0 and info["persistent_workgroups"] == 0 and same_bits(out, plain)


# ---------------------------------------------------------------------------------------------- shapes and edges
EDGE = (1, 127, 128, 129, 255, 257, 385)


@pytest.mark.parametrize("K", [0, 1, 3, 15, 16, 17, 31, 48, 100])
def test_shapes_and_edges(hip, K):
    """M, N in {1, 127, 128, 129, 255, 257, 385} crossed, every entry against the extended-precision reference; the
    epilogue options rotate over the 49 shapes so that each K sees every addend form and both triangle rules.
    K = 0: beta Cin (+ dvec) alone, zeros without an addend."""
    worst = 0.0
    n = 0
    for M in EDGE:
        for N in EDGE:
            cin = ("none", "sep", "alias")[n % 3]
            p = Problem(1000 * M + 10 * N + K, M, N, K, lower=(n // 3) % 2, cin=cin, dvec=(n % 4 == 1),
                        alpha=(1.0, -1.0, 0.5)[n % 3], beta=(1.0, -2.0)[n % 2])
            n += 1
            rc, info, out, prior = run(hip, p)
            assert rc == 0
            r64, rld = check(p, out, prior, info, f"edge M{M} N{N} K{K}")
            worst = max(worst, rld)
            if K == 0 and cin == "none" and p.dvec is None:
                W = p.written()
                assert np.all(out[:N, :M].T[W] == 0.0)
    print(f"[gemm-paths] shapes K {K}: worst err/bound {worst:.3e}")


def test_empty_products_write_nothing(hip):
    for M, N in ((0, 5), (5, 0), (0, 0)):
        p = Problem(5, M, N, 7)
        rc, info, out, prior = run(hip, p)
        assert rc == 0 and info["ntiles"] == 0 and info["segments"] == 0
        assert same_bits(out, prior)


@pytest.mark.parametrize("cin", ["none", "sep", "alias"])
def test_epilogue(hip, cin):
    """alpha in {1, -1, 0.5} x beta in {1, -2, 0} with the addend absent, separate (ldcin != ldc) and aliasing C, on a
    non-square product with partial edge tiles.  With an addend the kernel computes alpha acc + beta Cin as written: a
    FINITE Cin at beta = 0 gives alpha acc (pinned here; a NaN there would propagate, unlike BLAS)."""
    for alpha in (1.0, -1.0, 0.5):
        for beta in (1.0, -2.0, 0.0):
            p = Problem(int(alpha * 10) + int(beta * 100) + 1000, 300, 200, 72, alpha=alpha, beta=beta, cin=cin, dvec=True)
            rc, info, out, prior = run(hip, p)
            assert rc == 0
            check(p, out, prior, info, f"epilogue {cin} alpha {alpha} beta {beta}")
            if beta == 0.0 and cin != "none":
                q = Problem(int(alpha * 10) + int(beta * 100) + 1000, 300, 200, 72, alpha=alpha, beta=beta, cin="none", dvec=True)
                q.dvec = p.dvec
                _, _, out0, _ = run(hip, q)
                W = p.written()
                assert np.array_equal(out[:200, :300].T[W], out0[:200, :300].T[W]), "beta = 0 with a finite addend: alpha acc"
    # X and Y one array (the assembly's form)
    p = Problem(4, 257, 257, 40, lower=1, y_is_x=True, cin=cin, dvec=True)
    rc, info, out, prior = run(hip, p)
    assert rc == 0
    check(p, out, prior, info, f"epilogue {cin} X is Y")


@pytest.mark.parametrize("diag_off", [0, 128, -128, 37])
@pytest.mark.parametrize("lower", [0, 1])
def test_diagonal_offset(hip, diag_off, lower):
    """dvec lands where i + diag_off == j, and lower_only writes exactly the entries with i + diag_off >= j, on a
    non-square product -- also for an offset that is not a multiple of the tile (the table's tile-skip rule
    "last row of the tile + diag_off < first column" is exact for every offset, so 37 is computed, not refused) and for
    one (-128) that leaves the whole first tile row inactive.  K = 528 with few tiles: the split form and its reduce
    kernel's own diagonal rule; K = 40: the plain epilogue's second pass."""
    for K, form in ((40, dict(ksplit=one)), (528, dict(ksplit=ge2))):
        for M, N in ((385, 300), (300, 385)):
            p = Problem(diag_off + 1000 + K + M, M, N, K, lower=lower, diag_off=diag_off, cin="sep", dvec=True)
            rc, info, out, prior = run(hip, p)
            assert rc == 0, hip.lib.madqp_last_error(hip.ctx)
            expect(info, f"diag_off {diag_off} K {K}", **form)
            if lower and diag_off == -128:
                assert not p.written()[:128].any()
                full = ((M + 127) // 128) * ((N + 127) // 128)
                assert info["ntiles"] < full - 2  # (the first tile row and the tiles above the rule are not launched)
            check(p, out, prior, info, f"diag_off {diag_off} lower {lower} M{M} N{N} K{K}")


@pytest.mark.parametrize("K", [64, 100])
def test_fast_and_guarded_staging(hip, K):
    """Operands padded to a multiple of 128 rows (Mread / Nread) with finite garbage in the padding: edge tiles take
    the LDS-DMA loop, stores stay masked to M x N and the garbage does not leak in.  Pointers 8 bytes off a 16-byte
    boundary and odd leading dimensions (fast_ok = 0) take the register-staged loop on every tile.  Both loops consume k
    in the same order (module docstring), so for K % 16 == 0 the three results are bitwise equal; for K = 100 every
    tile is staged anyway and they are equal as well."""
    M, N = 300, 427
    base = Problem(K, M, N, K, cin="sep", dvec=True, ldx=392, ldy=524)
    padded = copy.copy(base)
    padded.Mread, padded.Nread = 384, 512
    odd = copy.copy(base)  # the same numbers at odd leading dimensions
    odd.X, odd.ldx = np.ascontiguousarray(base.X[:, :391]), 391
    odd.Y, odd.ldy = np.ascontiguousarray(base.Y[:, :523]), 523
    outs = {}
    for name, p, shift, fast in (("padded", padded, 0, 1), ("plain", base, 0, 1), ("shifted", base, 1, 0), ("odd_ld", odd, 0, 0)):
        rc, info, out, prior = run(hip, p, shift=shift)
        assert rc == 0
        assert info["fast_ok"] == fast, (name, info)
        check(p, out, prior, info, f"staging {name} K{K}")
        outs[name] = out
    for name in ("plain", "shifted", "odd_ld"):
        assert same_bits(outs[name], outs["padded"]), f"{name} and padded differ (K = {K})"


# ------------------------------------------------------------------------------------- masks and the table cache
def test_column_masks_and_the_table_cache(hip):
    """cols: each call writes exactly its column ranges, and those columns are bitwise the unmasked call's -- three calls
    on one shape with two masks (the cached tile table of a shape is keyed by the mask: the second mask must not get
    the first one's table, the third call must get the first one's again)."""
    p = Problem(9, 512, 512, 96, cin="sep", dvec=True)
    rc, info, whole, prior = run(hip, p)
    assert rc == 0 and info["ntiles"] == 16
    check(p, whole, prior, info, "mask/unmasked")
    for cols in ((0, 128, 384, 512), (128, 256, 384, 512), (0, 128, 384, 512), (0, 512)):
        rc, info, out, prior = run(hip, p, cols=cols)
        assert rc == 0
        assert info["ntiles"] == 4 * sum(b - a for a, b in zip(cols[0::2], cols[1::2])) // 128
        check(p, out, prior, info, f"mask/cols {cols}", cols=cols)
        W = p.written(cols)
        assert same_bits(out[:512, :512].T[W], whole[:512, :512].T[W])
    # lower triangle + mask, ragged last column range (a range may end at N)
    p = Problem(10, 700, 700, 50, lower=1, cin="alias", dvec=True)
    rc, info, whole, prior = run(hip, p)
    for cols in ((128, 256, 640, 700), (0, 128, 256, 384)):
        rc, info, out, prior = run(hip, p, cols=cols)
        assert rc == 0
        check(p, out, prior, info, f"mask/lower cols {cols}", cols=cols)
        W = p.written(cols)
        assert same_bits(out[:700, :700].T[W], whole[:700, :700].T[W])


def test_tile_row0_masks(hip):
    """tile_row0 (block-cyclic local matrices): tile column t is computed from tile row tile_row0[t] down, whole tiles;
    two arrays on one shape, then the first again."""
    p = Problem(11, 600, 512, 80, cin="sep")
    rc, info, whole, prior = run(hip, p)
    assert rc == 0 and info["ntiles"] == 20
    for rows in ((0, 1, 2, 5), (3, 0, 4, 1), (0, 1, 2, 5)):
        rc, info, out, prior = run(hip, p, tile_row0=rows)
        assert rc == 0
        assert info["ntiles"] == sum(5 - r for r in rows)
        check(p, out, prior, info, f"tile_row0 {rows}", tile_row0=rows)
        W = p.written(tile_row0=rows)
        assert same_bits(out[:512, :600].T[W], whole[:512, :600].T[W])


def test_malformed_masks_are_refused(hip):
    p = Problem(12, 512, 512, 16)
    for cols in ((0, 100), (64, 128), (0, 640), (-128, 128)):
        rc, info, out, prior = run(hip, p, cols=cols)
        assert rc == ERR_ARG, cols
        assert same_bits(out, prior)
    rc, _, out, prior = run(hip, p, cols=(0, 128), tile_row0=(0, 0, 0, 0))
    assert rc == ERR_ARG and same_bits(out, prior)
    q = Problem(12, 512, 512, 16, lower=1)
    rc, _, out, prior = run(hip, q, tile_row0=(0, 0, 0, 0))
    assert rc == ERR_ARG and same_bits(out, prior)
    rc, info = seam(hip, M=4, N=4, K=4, ldx=4, ldy=4, ldc=4)  # null operands
    assert rc == ERR_ARG


# ---------------------------------------------------------------------------------------------------------- batch
def _batch(hip, nprob, M, N, K, seed):
    """nprob problems of one shape stacked at fixed strides; returns the problems, the device arrays and, per problem,
    the result of the same product run ALONE through the seam."""
    ps = [Problem(seed + b, M, N, K, cin="sep", dvec=True) for b in range(nprob)]
    p0 = ps[0]
    Xs = G.dev(np.stack([p.X for p in ps]), hip)
    Ys = G.dev(np.stack([p.Y for p in ps]), hip)
    Cins = G.dev(np.stack([p.Cin for p in ps]), hip)
    Ds = G.dev(np.stack([p.dvec for p in ps]), hip)
    alone = []
    for p in ps:
        rc, info, out, prior = run(hip, p)
        assert rc == 0 and info["ksplit"] == 1 and info["batch_xcd"] == 0
        check(p, out, prior, info, f"batch/alone {len(alone)}")
        alone.append(out)
    f = dict(X=Xs, ldx=p0.ldx, Y=Ys, ldy=p0.ldy, ldc=p0.ldc, Cin=Cins, ldcin=p0.ldcin, dvec=Ds, alpha=p0.alpha, beta=p0.beta,
             M=M, N=N, K=K, sX=p0.X.size, sY=p0.Y.size, sC=N * p0.ldc, sCin=p0.Cin.size, sD=N)
    return ps, f, alone


def _batch_run(hip, f, nprob, N, ldc, **kw):
    Cd = torch.full((nprob, N, ldc), float("nan"), dtype=torch.float64, device=hip.device)
    rc, info = seam(hip, C=Cd, **f, **kw)
    assert rc == 0, hip.lib.madqp_last_error(hip.ctx)
    return info, Cd.cpu().numpy()


def _batch_assert(out, alone, done, label):
    nan = np.full_like(alone[0], np.nan)
    for b in range(len(out)):
        if b in done:
            assert same_bits(out[b], alone[b]), f"{label}: problem {b} differs from the same product run alone"
        else:
            assert same_bits(out[b], nan), f"{label}: problem {b} was written"


def test_batch_plain_and_xcd_redeal(hip):
    """B = 3 (grid.y = problem) and B = 16 (problems dealt to the XCDs whole, 9 tiles each: not a multiple of 8), with
    and without a skip list: every problem bitwise the same product run alone, skipped problems untouched."""
    M, N, K = 300, 290, 100
    ps, f, alone = _batch(hip, 16, M, N, K, 500)
    ldc = ps[0].ldc
    info, out = _batch_run(hip, f, 3, N, ldc, B=3)
    assert info["ntiles"] == 9 and info["batch_xcd"] == 0 and info["ksplit"] == 1
    _batch_assert(out, alone, {0, 1, 2}, "B = 3")
    info, out = _batch_run(hip, f, 16, N, ldc, B=16)
    assert info["batch_xcd"] == 1 and info["ntiles"] == 9, info
    _batch_assert(out, alone, set(range(16)), "B = 16")
    skipped = {1, 6, 7, 8, 15}
    skip = G.i32dev([1 if b in skipped else 0 for b in range(16)], hip)
    info, out = _batch_run(hip, f, 16, N, ldc, B=16, skip=skip)
    assert info["batch_xcd"] == 1
    _batch_assert(out, alone, set(range(16)) - skipped, "B = 16 with skip")
    skip3 = G.i32dev([0, 1, 0], hip)
    info, out = _batch_run(hip, f, 3, N, ldc, B=3, skip=skip3)
    _batch_assert(out, alone, {0, 2}, "B = 3 with skip")


def test_batch_of_one_honours_its_skip_word(hip):
    """A batch of ONE with a skip list is still a batch (gemm_select's comment records the round in which it was not)."""
    M, N, K = 257, 140, 48
    ps, f, alone = _batch(hip, 1, M, N, K, 600)
    for word, done in ((1, set()), (0, {0})):
        info, out = _batch_run(hip, f, 1, N, ps[0].ldc, B=1, skip=G.i32dev([word], hip))
        _batch_assert(out, alone, done, f"B = 1 skip {word}")


@pytest.mark.parametrize("count", [0, 3, 4, 9])
def test_batch_compacted_list(hip, count):
    """list / count with 4 slots: slot y works off list[y], list[y + 4], .. < count; unlisted problems keep their NaN."""
    M, N, K = 200, 260, 64
    ps, f, alone = _batch(hip, 12, M, N, K, 700)
    order = [7, 2, 11, 0, 5, 9, 3, 10, 1, 4, 6, 8]  # (entries past count are never read as problems)
    info, out = _batch_run(hip, f, 12, N, ps[0].ldc, B=4, list=G.i32dev(order, hip), count=G.i32dev([count], hip))
    assert info["batch_xcd"] == 0 and info["ntiles"] == 6
    _batch_assert(out, alone, set(order[:count]), f"list count {count}")


# ------------------------------------------------------------------------- variants chosen by environment knobs
def _child(names, env):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    p = subprocess.run([sys.executable, os.path.join(root, "tests", "gemm_paths.py")] + list(names),
                       env=dict(os.environ, **env), capture_output=True, text=True, timeout=900)
    sys.stdout.write("".join(l + "\n" for l in p.stdout.splitlines() if l.startswith("[gemm-paths]")))
    assert p.returncode == 0, (env, p.stdout[-1500:], p.stderr[-3000:])
    return json.loads(p.stdout.strip().splitlines()[-1])


def test_environment_variants_in_child_processes():
    """MADQP_GEMM_SEG_ROUNDS, MADQP_GEMM_XCD and MADQP_GEMM_SPLITK are read once per process: one child per variant, one
    after the other, none started after one has failed.  Every child holds its outputs to the references itself
    (tests/gemm_paths.py: child_case) and prints their SHA-256 and the dispatcher's report.  Segmented launches and the
    launch without the XCD remap give the bytes of the default launch; without split-K the split cases agree within the
    bound (another order of summation), which the child's own check asserts."""
    base = _child(("seg2", "seg5", "seg_merge", "split", "tail"), {})
    for n in ("seg2", "seg5", "seg_merge"):
        expect(base[n]["info"], f"default/{n}", segments=one, ksplit=one, tail_tiles=zero)
    expect(base["split"]["info"], "default/split", ksplit=ge2)
    expect(base["split"]["info"], "default/split", ksplit=14, ntiles=36)
    expect(base["tail"]["info"], "default/tail", tail_tiles=pos, tail_split=ge2)

    seg = _child(("seg2", "seg5", "seg_merge"), {"MADQP_GEMM_SEG_ROUNDS": "1"})
    for n, count, tiles in (("seg2", 2, 820), ("seg5", 5, 2556), ("seg_merge", 2, 1081)):
        expect(seg[n]["info"], f"SEG_ROUNDS=1/{n}", segments=ge2)
        expect(seg[n]["info"], f"SEG_ROUNDS=1/{n}", segments=count, ntiles=tiles)  # 512 + 308 | 4 x 512 + 508 | 512 + 569
        assert seg[n]["sha"] == base[n]["sha"], f"segmented launch of {n} differs from the single launch"

    flat = _child(("seg2", "split", "tail"), {"MADQP_GEMM_XCD": "0"})
    for n in ("seg2", "split", "tail"):
        assert flat[n]["info"] == base[n]["info"]
        assert flat[n]["sha"] == base[n]["sha"], f"{n} without the XCD remap differs: the tile-to-workgroup map entered the result"

    whole = _child(("split", "tail"), {"MADQP_GEMM_SPLITK": "0"})
    for n in ("split", "tail"):
        expect(whole[n]["info"], f"SPLITK=0/{n}", ksplit=one, tail_tiles=zero, segments=one)
