"""The launch plan and the tile table of the fp64 MFMA product (madqp_jl_amd/csrc/gemm_plan.inc, compiled for the CPU by
tests/csrc): what madqp_gemm_tn launches for a given tile count, K, number of resident workgroups and switches, held by
explicit figures -- the dispatches tests/test_gpu_gemm_paths.py records on a device, and both sides of every constant of
the rules -- and the order of the tile table.  No GPU.  Figures are for 512 resident workgroups unless a case says so."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T = 128
SINGLE, BATCH, BATCH_LIST = 0, 1, 2
NONE, COLS, ROW0 = 0, 1, 2
FIELDS = ("ntiles", "whole", "ksplit", "kchunk", "segments", "tail_tiles", "tail_split", "tail_chunk", "persistent",
          "batch_xcd", "gy", "work_bytes")
MODES = ("splitk", "tailsplit", "seg_rounds", "xcd", "batch_xcd", "patch_m", "patch_n")


@pytest.fixture(scope="module")
def lib():
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "tests", "csrc")], stdout=subprocess.DEVNULL)
    lib = C.CDLL(os.path.join(ROOT, "tests", "_build", "libmadqp_gemm_plan.so"))
    lib.gemm_plan_c.restype = None
    lib.gemm_plan_c.argtypes = [C.c_int64] * 4 + [C.c_int, C.c_int64] + [C.c_void_p] * 3 + [C.c_int64]
    lib.gemm_tile_table_c.restype = C.c_int64
    lib.gemm_tile_table_c.argtypes = [C.c_int64, C.c_int64, C.c_int, C.c_int64, C.c_int, C.c_void_p, C.c_int64, C.c_void_p,
                                      C.c_void_p, C.c_int64]
    lib.gemm_default_modes_c.restype = None
    lib.gemm_default_modes_c.argtypes = [C.c_void_p]
    return lib


def modes_array(lib, modes):
    m = np.zeros(7, dtype=np.int64)
    lib.gemm_default_modes_c(m.ctypes.data)
    for k, v in modes.items():
        m[MODES.index(k)] = v
    return m


def plan(lib, ntiles, K, *, slots=512, cap=0, form=SINGLE, B=1, **modes):
    """The plan as a dict of FIELDS, plus "segs": the tiles of each segment."""
    out = np.zeros(12, dtype=np.int64)
    segs = np.zeros(4096, dtype=np.int64)
    m = modes_array(lib, modes)
    lib.gemm_plan_c(ntiles, K, slots, cap, form, B, m.ctypes.data, out.ctypes.data, segs.ctypes.data, len(segs))
    p = dict(zip(FIELDS, (int(v) for v in out)))
    p["segs"] = [int(s) for s in segs[:p["segments"]]]
    assert sum(p["segs"]) == (p["whole"] if p["segments"] else 0)
    assert p["whole"] + p["tail_tiles"] == p["ntiles"] == ntiles
    return p


def table(lib, M, N, lower=0, diag_off=0, kind=NONE, mask=(), **modes):
    """The tile table as a list of (tile row, tile column)."""
    mk = np.asarray(mask, dtype=np.int64)
    out = np.zeros(((M + T - 1) // T) * ((N + T - 1) // T) + 1, dtype=np.int32)
    n = lib.gemm_tile_table_c(M, N, lower, diag_off, kind, mk.ctypes.data, len(mk), modes_array(lib, modes).ctypes.data,
                              out.ctypes.data, len(out))
    assert 0 <= n < len(out)
    return [(int(e) >> 16, int(e) & 0xFFFF) for e in out[:n]]


def whole(n, segs=None):
    return dict(ntiles=n, whole=n, ksplit=1, tail_tiles=0, tail_split=0, persistent=0, work_bytes=0, gy=1,
                segs=[n] if segs is None else segs)


def split(n, S, chunk):
    return dict(ntiles=n, whole=n, ksplit=S, kchunk=chunk, tail_tiles=0, persistent=0, segs=[n], gy=S,
                work_bytes=S * n * T * T * 8)


def tail(n_whole, n_tail, S, chunk):
    return dict(ntiles=n_whole + n_tail, whole=n_whole, ksplit=1, tail_tiles=n_tail, tail_split=S, tail_chunk=chunk,
                persistent=0, segs=[n_whole], gy=1, work_bytes=S * n_tail * T * T * 8)


def holds(p, want, label):
    for k, v in want.items():
        assert p[k] == v, f"{label}: {k} = {p[k]}, expected {v}: {p}"
    if p["ksplit"] == 1:
        assert p["kchunk"] == label[1], f"{label}: an unsplit launch walks all of K: {p}"


# ------------------------------------------------------------------------------------------- (a) recorded dispatches
# (M, N, K, lower) -> plan: the PATHS table of tests/test_gpu_gemm_paths.py
RECORDED = [
    ((300, 300, 600, 1), split(6, 2, 304)),
    ((1000, 1000, 5000, 1), split(36, 14, 368)),
    ((2300, 640, 1660, 0), split(90, 5, 336)),
    ((2800, 2800, 520, 1), split(253, 2, 272)),
    ((5000, 5000, 2000, 1), tail(512, 308, 3, 672)),
    ((5000, 5000, 2016, 1), tail(512, 308, 3, 672)),
    ((4000, 4000, 1024, 1), tail(512, 16, 4, 256)),
    ((7000, 7000, 1500, 1), tail(1536, 4, 5, 304)),
    ((5000, 5000, 8192, 1), split(820, 3, 2736)),
    ((6000, 6000, 6000, 1), split(1128, 2, 3008)),
    ((3000, 3000, 4100, 1), whole(300)),
    ((5000, 1280, 3720, 0), whole(400)),
]


@pytest.mark.parametrize("shape,want", RECORDED, ids=["x".join(map(str, s)) for s, _ in RECORDED])
def test_recorded_dispatches(lib, shape, want):
    M, N, K, lower = shape
    ntiles = len(table(lib, M, N, lower))
    holds(plan(lib, ntiles, K), want, (shape, K))


def test_recorded_segments_and_persistent_launches(lib):
    for (M, K), segs in (((5000, 512), [512, 308]), ((9000, 64), [512] * 4 + [508]), ((5888, 64), [512, 569])):
        n = len(table(lib, M, M, 1))
        assert n == sum(segs)
        holds(plan(lib, n, K, seg_rounds=1), whole(n, segs), ((M, K, "SEG_ROUNDS=1"), K))
        holds(plan(lib, n, K), whole(n), ((M, K), K))
        holds(plan(lib, n, K, seg_rounds=0), whole(n), ((M, K, "SEG_ROUNDS=0"), K))
    for cap, wgs in ((128, 384), (500, 8)):
        p = plan(lib, 820, 512, cap=cap)
        holds(p, dict(persistent=wgs, segments=0, segs=[], ksplit=1, tail_tiles=0, whole=820, work_bytes=0), ((cap,), 512))


# --------------------------------------------------------------------------------- (b) both sides of every constant
def test_split_of_few_tiles(lib):
    holds(plan(lib, 253, 511), whole(253), ("K = 511", 511))                 # K >= 512
    holds(plan(lib, 253, 512), split(253, 2, 256), ("K = 512", 512))
    holds(plan(lib, 256, 1024), split(256, 2, 512), ("256 tiles", 1024))     # 2 ntiles <= slots
    holds(plan(lib, 257, 1024), whole(257), ("257 tiles", 1024))
    holds(plan(lib, 170, 1024), split(170, 3, 352), ("170 tiles", 1024))     # S = slots / ntiles
    holds(plan(lib, 171, 1024), split(171, 2, 512), ("171 tiles", 1024))
    holds(plan(lib, 8, 767), split(8, 2, 384), ("K = 767", 767))             # S = K / 256
    holds(plan(lib, 8, 768), split(8, 3, 256), ("K = 768", 768))
    holds(plan(lib, 8, 38000), split(8, 16, 2384), ("K = 38000", 38000))     # S <= 16
    holds(plan(lib, 32, 4096), split(32, 16, 256), ("32 tiles", 4096))
    # the chunk is rounded up to the stage of 16: 257 -> 272, of which 15 reach 4080 only
    holds(plan(lib, 8, 4097), split(8, 16, 272), ("K = 4097", 4097))


def test_split_of_a_few_rounds_of_long_tiles(lib):
    # K >= 4096; at 820 tiles two chunks of 2048 do not pay and the tail rule takes over on both sides
    holds(plan(lib, 820, 4095), tail(512, 308, 3, 1376), ("820 tiles", 4095))
    holds(plan(lib, 820, 4096), tail(512, 308, 3, 1376), ("820 tiles", 4096))
    # at 600 tiles (2 rounds as they are, 3 rounds of half the length in two chunks) they do
    holds(plan(lib, 600, 4095), tail(512, 88, 5, 832), ("600 tiles", 4095))
    holds(plan(lib, 600, 4096), split(600, 2, 2048), ("600 tiles", 4096))
    # K / S >= 2048: three chunks need K >= 6144
    holds(plan(lib, 820, 6143), tail(512, 308, 3, 2048), ("820 tiles", 6143))
    holds(plan(lib, 820, 6144), split(820, 3, 2048), ("820 tiles", 6144))
    # 2 ntiles > slots: 256 tiles are "few tiles" (S = 2, one chunk per workgroup that is there), 257 a round of long
    # tiles (three chunks in two rounds of a third)
    holds(plan(lib, 256, 8192), split(256, 2, 4096), ("256 tiles", 8192))
    holds(plan(lib, 257, 8192), split(257, 3, 2736), ("257 tiles", 8192))
    # S <= 16: 513 tiles of K = 40000 in 17 rounds of a sixteenth; 257 tiles of K = 50000 would fill 9 rounds of a
    # seventeenth and take 8 rounds of a fifteenth
    holds(plan(lib, 513, 40000), split(513, 16, 2512), ("513 tiles", 40000))
    holds(plan(lib, 257, 50000), split(257, 15, 3344), ("257 tiles", 50000))
    # ntiles < 8 slots: 7.03 rounds (that take 8) are 43 rounds of a sixth; 8 rounds less one tile are 8 S rounds in S
    # chunks, never worth it, so at the bound itself both sides are whole
    holds(plan(lib, 3600, 38000), split(3600, 6, 6336), ("3600 tiles", 38000))
    holds(plan(lib, 8 * 512 - 1, 38000), whole(4095), ("8 slots - 1", 38000))
    holds(plan(lib, 8 * 512, 38000), whole(4096), ("8 slots", 38000))
    # past the bound the rule is off however well a split would pay: nine rounds with one tile in the last, which two
    # chunks would run as 17 half rounds (70 348 against 74 167 us by the model)
    holds(plan(lib, 8 * 512 + 1, 38000), whole(4097), ("8 slots + 1", 38000))
    holds(plan(lib, 3925, 38000), split(3925, 3, 12672), ("3925 tiles", 38000))   # 23 rounds of a third for 8
    holds(plan(lib, 3926, 38000), whole(3926), ("3926 tiles", 38000))             # 24
    # must beat 0.97 of the launch as it is.  Model cost of the best split / cost as it is:
    #   3840 tiles of K = 5120, two chunks: 15 rounds of 563 us + 384 against 8 of 1116 + 192: 0.9681 -- split
    #   2305 tiles of K = 8192, three chunks: 14 rounds of 600 us + 346 against 5 of 1779 + 115: 0.9701 -- whole
    holds(plan(lib, 3840, 5120), split(3840, 2, 2560), ("3840 tiles", 5120))
    holds(plan(lib, 2305, 8192), whole(2305), ("2305 tiles", 8192))
    # a tile more is a round more of thirds: 1365 tiles of K = 8192 in 8 rounds of a third for 3 (0.925); 1366 tiles are
    # best in four chunks, 11 rounds of a quarter (0.9709), and stay whole; so do 3585 of K = 4096 (0.9737)
    holds(plan(lib, 1365, 8192), split(1365, 3, 2736), ("1365 tiles", 8192))
    holds(plan(lib, 1366, 8192, tailsplit=0), whole(1366), ("1366 tiles", 8192))
    holds(plan(lib, 3585, 4096), whole(3585), ("3585 tiles", 4096))
    holds(plan(lib, 1000, 4096, tailsplit=0), whole(1000), ("1000 tiles", 4096))  # 4 half rounds for 2: 1.03


def test_tail_split(lib):
    holds(plan(lib, 528, 1023), whole(528), ("K = 1023", 1023))              # K >= 1024
    holds(plan(lib, 528, 1024), tail(512, 16, 4, 256), ("K = 1024", 1024))
    # 10 tl < 8 slots, on 20 workgroups where the bound is a whole number of tiles: 15 and 16 tiles in the last round
    holds(plan(lib, 35, 4000, slots=20), tail(20, 15, 4, 1008), ("tl = 15 of 20", 4000))
    holds(plan(lib, 36, 4000, slots=20), whole(36), ("tl = 16 of 20", 4000))
    # slots < ntiles < 4 slots: a last round of 511 is too full on either side of the upper bound, one of 16 is not
    holds(plan(lib, 4 * 512 - 1, 1024), whole(2047), ("4 slots - 1", 1024))
    holds(plan(lib, 4 * 512, 1024), whole(2048), ("4 slots", 1024))
    holds(plan(lib, 3 * 512 + 16, 1024), tail(1536, 16, 4, 256), ("3 slots + 16", 1024))
    holds(plan(lib, 4 * 512 + 16, 1024), whole(2064), ("4 slots + 16", 1024))
    holds(plan(lib, 512, 2000), whole(512), ("one full round", 2000))
    holds(plan(lib, 513, 2000), tail(512, 1, 7, 288), ("one round and a tile", 2000))
    # S <= 8 with K / S >= 256: four tiles of K = 1500 take 5 chunks (PATHS), of K = 1279 four, of K = 38000 eight
    holds(plan(lib, 1540, 1279), tail(1536, 4, 4, 320), ("K = 1279", 1279))
    holds(plan(lib, 1540, 1280), tail(1536, 4, 5, 256), ("K = 1280", 1280))
    holds(plan(lib, 516, 3000), tail(512, 4, 8, 384), ("K = 3000", 3000))
    # a clear gain only: the split tail must beat 0.93 of one whole piece (231 us at K = 1024, 442 us at K = 2000).
    # Three chunks of 316 tiles are 2 rounds of 83.7 us + 47.4 = 0.9294, of 317 tiles + 47.55 = 0.9300 (above)
    holds(plan(lib, 512 + 316, 1024), tail(512, 316, 3, 352), ("tl = 316", 1024))
    holds(plan(lib, 512 + 317, 1024), whole(829), ("tl = 317", 1024))
    # 341 tiles in three chunks fill 2 rounds (0.813), 342 need a third, or four chunks in 3 rounds (0.956)
    holds(plan(lib, 512 + 341, 2000), tail(512, 341, 3, 672), ("tl = 341", 2000))
    holds(plan(lib, 512 + 342, 2000), whole(854), ("tl = 342", 2000))
    holds(plan(lib, 912, 2000), whole(912), ("tl = 400", 2000))
    # not beside a capped launch, which is persistent instead
    holds(plan(lib, 820, 2000, cap=128), dict(persistent=384, segments=0, tail_tiles=0, ksplit=1, whole=820, work_bytes=0),
          ("cap 128", 2000))
    # the persistent launch needs more whole tiles than workgroups, a cap leaves at least 8 workgroups
    holds(plan(lib, 384, 64, cap=128), whole(384), ("384 tiles on 384", 64))
    holds(plan(lib, 385, 64, cap=128), dict(persistent=384, segments=0), ("385 tiles on 384", 64))
    holds(plan(lib, 385, 64, cap=135), dict(persistent=376, segments=0), ("cap 135", 64))
    holds(plan(lib, 9, 64, cap=511), dict(persistent=8, segments=0), ("cap 511", 64))
    holds(plan(lib, 36, 5000, cap=500), split(36, 14, 368), ("a split launch is not capped", 5000))


def test_switches_and_batches(lib):
    holds(plan(lib, 36, 5000, splitk=0), whole(36), ("SPLITK=0", 5000))
    holds(plan(lib, 820, 8192, splitk=0), whole(820), ("SPLITK=0", 8192))
    holds(plan(lib, 528, 1024, splitk=0), whole(528), ("SPLITK=0", 1024))
    holds(plan(lib, 528, 1024, tailsplit=0), whole(528), ("TAILSPLIT=0", 1024))
    holds(plan(lib, 36, 5000, tailsplit=0), split(36, 14, 368), ("TAILSPLIT=0", 5000))
    for form, B, gy, xcd in ((BATCH, 3, 3, 0), (BATCH, 16, 16, 1), (BATCH, 8, 8, 1), (BATCH, 12, 12, 0), (BATCH, 1, 1, 0),
                             (BATCH, 0, 1, 0), (BATCH_LIST, 16, 16, 0), (BATCH_LIST, 4, 4, 0)):
        for n, K in ((36, 5000), (820, 8192), (528, 1024), (820, 2000)):  # every split is off for a batch
            holds(plan(lib, n, K, form=form, B=B), dict(whole(n), gy=gy, batch_xcd=xcd), ((form, B, n), K))
        holds(plan(lib, 820, 512, form=form, B=B, cap=128), dict(whole(820), gy=gy), ((form, B, "cap"), 512))
    holds(plan(lib, 9, 100, form=BATCH, B=16, batch_xcd=0), dict(whole(9), gy=16, batch_xcd=0), ("BATCH_XCD=0", 100))
    holds(plan(lib, 9, 100, form=SINGLE, B=16), dict(whole(9), gy=1, batch_xcd=0), ("no batch", 100))
    holds(plan(lib, 2556, 64, form=BATCH, B=3, seg_rounds=1), dict(whole(2556, [512] * 4 + [508]), gy=3), ("batch in segments", 64))


def test_segments(lib):
    # a remainder shorter than a quarter of a segment joins the one before
    holds(plan(lib, 2 * 512 + 127, 64, seg_rounds=1), whole(1151, [512, 639]), ("seg / 4 - 1", 64))
    holds(plan(lib, 2 * 512 + 128, 64, seg_rounds=1), whole(1152, [512, 512, 128]), ("seg / 4", 64))
    holds(plan(lib, 512 + 127, 64, seg_rounds=1), whole(639, [639]), ("one segment and a bit", 64))
    holds(plan(lib, 3 * 512, 64, seg_rounds=1), whole(1536, [512] * 3), ("three whole segments", 64))
    holds(plan(lib, 64 * 512 + 8191, 64), whole(40959), ("64 rounds and less than 16", 64))
    holds(plan(lib, 64 * 512 + 8192, 64), whole(40960, [32768, 8192]), ("64 + 16 rounds", 64))
    holds(plan(lib, 5 * 512, 64, seg_rounds=2), whole(2560, [1024, 1024, 512]), ("SEG_ROUNDS=2", 64))
    # the whole tiles of a tail split are what is segmented; the tail is one launch
    holds(plan(lib, 1540, 1500, seg_rounds=1), dict(tail(1536, 4, 5, 304), segs=[512] * 3), ("tail in segments", 1500))
    # a launch cut in K is one launch (its partial tiles are indexed by its own tile count)
    holds(plan(lib, 820, 8192, seg_rounds=1), split(820, 3, 2736), ("split, SEG_ROUNDS=1", 8192))


def test_another_device(lib):
    """208 resident workgroups (104 CUs): no figures from such a device exist, the qualitative forms as
    tests/test_gpu_gemm_paths.py: expect() asserts them."""
    p = plan(lib, 36, 5000, slots=208)
    assert p["ksplit"] >= 2 and p["tail_tiles"] == 0 and p["segments"] == 1 and p["persistent"] == 0
    assert p["ksplit"] * 36 <= 208 and p["kchunk"] % 16 == 0 and (p["ksplit"] - 1) * p["kchunk"] < 5000 <= p["ksplit"] * p["kchunk"]
    p = plan(lib, 208 + 16, 1024, slots=208)
    assert p["ksplit"] == 1 and p["tail_tiles"] == 16 and p["whole"] == 208 and p["tail_split"] >= 2 and p["persistent"] == 0
    p = plan(lib, 330, 8192, slots=208)
    assert p["ksplit"] >= 2 and p["tail_tiles"] == 0 and p["persistent"] == 0 and p["kchunk"] >= 2048
    p = plan(lib, 300, 4100, slots=208, splitk=0)
    assert p["ksplit"] == 1 and p["tail_tiles"] == 0 and p["segments"] == 1
    p = plan(lib, 820, 512, slots=208, cap=100)
    assert p["persistent"] == 104 and p["segments"] == 0 and p["ksplit"] == 1 and p["tail_tiles"] == 0
    p = plan(lib, 820, 64, slots=208, seg_rounds=1)
    assert p["segs"] == [208, 208, 208, 196]


# ------------------------------------------------------------------------------------------------------ (c) tables
def test_table_literals(lib):
    assert table(lib, 300, 300, 1) == [(2, 0), (2, 1), (2, 2), (0, 0), (1, 0), (1, 1)]
    assert table(lib, 300, 300, 0) == [(2, 0), (2, 1), (2, 2), (0, 2), (1, 2), (0, 0), (1, 0), (0, 1), (1, 1)]
    assert table(lib, 256, 300, 0) == [(0, 2), (1, 2), (0, 0), (1, 0), (0, 1), (1, 1)]
    assert table(lib, 1, 1, 1) == [(0, 0)] and table(lib, 128, 128, 0) == [(0, 0)]
    assert table(lib, 129, 128, 1) == [(1, 0), (0, 0)]
    assert table(lib, 128, 129, 1) == [(0, 0)]  # (tile (0, 1) lies above the diagonal)
    assert table(lib, 384, 384, 1, -128) == [(1, 0), (2, 0), (2, 1)]  # the first tile row is inactive
    assert table(lib, 384, 384, 1, 128) == [(0, 0), (1, 0), (2, 0), (0, 1), (1, 1), (2, 1), (1, 2), (2, 2)]
    assert table(lib, 384, 384, 1, 37) == [(0, 0), (1, 0), (2, 0), (0, 1), (1, 1), (2, 1), (1, 2), (2, 2)]
    assert table(lib, 384, 384, 1, -1) == [(0, 0), (1, 0), (2, 0), (1, 1), (2, 1), (2, 2)]
    assert table(lib, 256, 512, 0, 0, COLS, (0, 128, 384, 512)) == [(0, 0), (1, 0), (0, 3), (1, 3)]
    assert table(lib, 256, 300, 0, 0, COLS, (128, 300)) == [(0, 2), (1, 2), (0, 1), (1, 1)]
    assert table(lib, 256, 512, 0, 0, COLS, ()) == []
    assert table(lib, 384, 384, 0, 0, ROW0, (0, 2, 3)) == [(0, 0), (1, 0), (2, 0), (2, 1)]
    # 9 x 9 tiles in patches of 8 x 8: the ninth tile row of the first eight columns follows the first patch's columns
    t = table(lib, 1152, 1152, 0)
    assert t[:9] == [(r, 0) for r in range(8)] + [(0, 1)] and t[64:66] == [(0, 8), (1, 8)] and t[72:74] == [(8, 0), (8, 1)]
    assert table(lib, 384, 256, 0, patch_m=2, patch_n=1) == [(0, 0), (1, 0), (0, 1), (1, 1), (2, 0), (2, 1)]


def masks_of(M, N, lower):
    tn = (N + T - 1) // T
    tm = (M + T - 1) // T
    yield NONE, ()
    yield COLS, [x for t in range(0, tn, 3) for x in (t * T, min(N, (t + 1) * T))]
    yield COLS, (T * (tn // 2), N)
    if not lower:
        yield ROW0, [(5 * t + 1) % (tm + 1) for t in range(tn)]


@pytest.mark.parametrize("lower", [0, 1])
def test_tables_hold_every_active_tile_once_in_order(lib, lower):
    sizes = (1, 128, 129, 300, 1100)
    for M in sizes:
        for N in sizes:
            for diag_off in (0, 128, -128, 37):
                for kind, mask in masks_of(M, N, lower):
                    tm_n, tn_n = (M + T - 1) // T, (N + T - 1) // T
                    on = np.ones(tn_n, dtype=bool)
                    if kind == COLS:
                        on[:] = False
                        for a, b in zip(mask[0::2], mask[1::2]):
                            on[a // T:(b + T - 1) // T] = True
                    active = {(i, j) for i in range(tm_n) for j in range(tn_n)
                              if on[j] and not (kind == ROW0 and i < mask[j])
                              and not (lower and i * T + T - 1 + diag_off < j * T)}
                    t = table(lib, M, N, lower, diag_off, kind, mask)
                    label = (M, N, lower, diag_off, kind, tuple(mask))
                    assert len(t) == len(set(t)) and set(t) == active, label
                    m_edge, n_edge = M % T != 0, N % T != 0
                    rows = [e for e in t if m_edge and e[0] == tm_n - 1]
                    cols = [e for e in t if n_edge and e[1] == tn_n - 1 and e not in rows]
                    rest = t[len(rows) + len(cols):]
                    assert t[:len(rows)] == sorted(rows, key=lambda e: e[1]), label  # the partial tile row first
                    assert t[len(rows):len(rows) + len(cols)] == sorted(cols), label   # then the partial tile column
                    # then 8 x 8 patches, row of patches by row of patches, column inside patch
                    assert rest == sorted(rest, key=lambda e: (e[0] // 8, e[1] // 8, e[1], e[0])), label
