"""CPU: the boundaries of the dense mat-vec dispatcher (csrc/gemv.hip: gemv_plan, the one function madqp_gemv launches
from) through the seam madqp_debug_gemv_form.  The seam touches no memory and no device, so the addresses are made up:
only their alignment matters.  Every constant of the rules is held from both sides by explicit figures -- the test does not
restate the rules, so a retuned threshold fails here by name and tests/test_gpu_matvec.py then says which kernel lost its
coverage.  (MADQP_GEMV_T_STRIP=0 in the environment switches the strip form off: the figures are those of the default.)"""
import pytest

import madqp_jl_amd as M
from matvec import ALIGNED, ERR_ARG, OFF8, form


@pytest.fixture(scope="module")
def lib():
    return M.load_cdll()


def q(lib, trans, rows, cols, lda=None, A=ALIGNED, x=ALIGNED):
    rc, d = form(lib, trans, rows, cols, A, cols + (cols & 1) if lda is None else lda, x)
    assert rc == 0, (trans, rows, cols, lda, rc)
    return d


def test_nothing_to_write_and_nothing_to_sum(lib):
    none = dict(form="none", vec=0, chunks=0, rows_per_chunk=0, workgroups=0)
    assert form(lib, 0, 0, 5, None, 0, None) == (0, none)
    assert form(lib, 1, 5, 0, None, 0, None) == (0, none)
    assert form(lib, 0, 0, 0, None, 0, None) == (0, none)
    # inner length 0: y = beta y, 256 entries per workgroup; A, x and lda are not looked at
    for trans, rows, cols in ((0, 5, 0), (1, 0, 5)):
        assert form(lib, trans, rows, cols, None, 0, None) == (0, dict(none, form="scale", workgroups=1))
    assert form(lib, 0, 256, 0, None, 0, None)[1]["workgroups"] == 1
    assert form(lib, 0, 257, 0, None, 0, None)[1]["workgroups"] == 2
    assert form(lib, 1, 0, 513, OFF8, 0, OFF8)[1] == dict(none, form="scale", workgroups=3)


def test_refusals(lib):
    for args in [(2, 4, 4, ALIGNED, 4, ALIGNED), (-1, 4, 4, ALIGNED, 4, ALIGNED), (0, -1, 4, ALIGNED, 4, ALIGNED),
                 (1, 4, -1, ALIGNED, 4, ALIGNED), (0, 4, 4, None, 4, ALIGNED), (1, 4, 4, ALIGNED, 4, None),
                 (0, 4, 4, ALIGNED, 3, ALIGNED), (1, 4, 4, ALIGNED, 3, ALIGNED)]:
        assert form(lib, *args)[0] == ERR_ARG, args
    assert lib.madqp_debug_gemv_form(0, 4, 4, ALIGNED, 4, ALIGNED, None) == ERR_ARG
    assert form(lib, 0, 4, 4, ALIGNED, 4, ALIGNED)[0] == 0


@pytest.mark.parametrize("rows,cols,want", [
    (1, 1, "n_wave"), (3, 1024, "n_wave"), (3, 1025, "n_block"), (2047, 1024, "n_wave"), (2047, 1025, "n_block"),
    (2048, 1025, "n_wave"), (2047, 100000, "n_block"), (2048, 100000, "n_wave"), (100000, 1024, "n_wave")])
def test_trans0_wave_or_block(lib, rows, cols, want):
    """rows >= 2048 || cols <= 1024: one wave per row; else one workgroup per row"""
    for lda, A, x in ((None, ALIGNED, ALIGNED), (cols | 1, OFF8, OFF8)):  # (the alignment does not move the rule)
        assert q(lib, 0, rows, cols, lda, A, x)["form"] == want


def test_trans0_workgroups(lib):
    """wave: four rows per workgroup, at most 8192 workgroups (then the rows are strided); block: one row per workgroup
    (its cap of 4096 cannot bind below 2048 rows)"""
    for rows, wg in ((1, 1), (4, 1), (5, 2), (32764, 8191), (32765, 8192), (32768, 8192), (32769, 8192), (10 ** 6, 8192)):
        assert q(lib, 0, rows, 3)["workgroups"] == wg, rows
    for rows in (1, 3, 2047):
        assert q(lib, 0, rows, 1025)["workgroups"] == rows
    assert q(lib, 0, 5, 3)["chunks"] == 0 and q(lib, 0, 5, 3)["rows_per_chunk"] == 0


@pytest.mark.parametrize("rows,cols", [(7, 65), (3, 1027)])  # (wave, block)
def test_trans0_vectorised_needs_A_x_and_an_even_lda(lib, rows, cols):
    ev = cols + 1
    assert q(lib, 0, rows, cols, ev)["vec"] == 1
    assert q(lib, 0, rows, cols, ev + 2)["vec"] == 1
    assert q(lib, 0, rows, cols, cols)["vec"] == 0           # lda odd
    assert q(lib, 0, rows, cols, ev, A=OFF8)["vec"] == 0
    assert q(lib, 0, rows, cols, ev, x=OFF8)["vec"] == 0      # x alone
    assert q(lib, 0, rows, cols, ev, A=ALIGNED + 16, x=ALIGNED + 32)["vec"] == 1
    assert q(lib, 0, rows, cols, ev, A=ALIGNED + 4)["vec"] == 0  # (any of the low four address bits)


def test_trans1_vectorised_needs_A_and_an_even_lda_only(lib):
    for rows, cols in ((5, 129), (131, 257)):  # (single, chunked)
        ev = cols + 1
        assert q(lib, 1, rows, cols, ev)["vec"] == 1
        assert q(lib, 1, rows, cols, cols)["vec"] == 0
        assert q(lib, 1, rows, cols, ev, A=OFF8)["vec"] == 0
        assert q(lib, 1, rows, cols, ev, x=OFF8)["vec"] == 1  # x is read double by double


def test_trans1_strip_window(lib):
    """vectorised && cols >= 2048 && 64 <= rows <= 16384 && rows * cols <= 2^27: 16 columns per workgroup"""
    strip = lambda *a, **k: q(lib, 1, *a, **k)["form"] == "t_strip"
    assert strip(64, 2048) and not strip(63, 2048) and not strip(64, 2047)
    assert strip(16384, 2048) and not strip(16385, 2048)
    assert strip(16384, 8192) and not strip(16384, 8193)       # rows * cols = 2^27 | 2^27 + 16384
    assert strip(8192, 16384) and not strip(8193, 16384)       # the same product bound, the rows moving
    assert strip(64, 2 ** 21) and not strip(64, 2 ** 21 + 1, 2 ** 21 + 2) and not strip(65, 2 ** 21)
    assert not strip(64, 2049, 2049) and strip(64, 2049, 2050)  # lda odd
    assert not strip(64, 2048, A=OFF8) and strip(64, 2048, x=OFF8)
    for cols, wg in ((2048, 128), (2049, 129), (2064, 129), (2065, 130)):
        d = q(lib, 1, 300, cols)
        assert (d["form"], d["vec"], d["chunks"], d["rows_per_chunk"], d["workgroups"]) == ("t_strip", 1, 1, 300, wg)


def test_trans1_chunks(lib):
    """128-column tiles x chunks of rows: min(ceil(2048 / tiles), rows / 64, 64) chunks of ceil(rows / chunks) rows rounded
    up to a multiple of 4, then as many chunks as that length needs"""
    t = lambda rows, cols, lda=None: (lambda d: (d["form"], d["chunks"], d["rows_per_chunk"], d["workgroups"]))(
        q(lib, 1, rows, cols, lda))
    # rows / 64: one chunk below 128 rows
    assert t(1, 1) == ("t_single", 1, 4, 1)
    assert t(127, 130) == ("t_single", 1, 128, 2)
    assert t(128, 130) == ("t_chunked", 2, 64, 4)
    assert t(191, 3) == ("t_chunked", 2, 96, 2) and t(192, 3) == ("t_chunked", 3, 64, 3)
    # the length of a chunk is a multiple of 4, and the count follows the rounded length
    assert t(131, 257) == ("t_chunked", 2, 68, 6)
    assert t(129, 3) == ("t_chunked", 2, 68, 2)  # 68 + 61 rows
    assert t(4100, 5) == ("t_chunked", 61, 68, 61)
    # tiles of 128 columns
    assert t(5, 128)[3] == 1 and t(5, 129)[3] == 2
    # at most 64 chunks
    assert t(4096, 5) == ("t_chunked", 64, 64, 64)     # rows / 64 = 64
    assert t(4352, 5) == ("t_chunked", 64, 68, 64)     # 68 -> 64
    assert t(8192, 5) == ("t_chunked", 64, 128, 64)    # 128 -> 64
    # ceil(2048 / tiles) binds from 33 tiles on (below the strip window only for a scalar product or many rows)
    assert t(6400, 4096, 4097) == ("t_chunked", 64, 100, 32 * 64)    # 32 tiles: 64
    assert t(6400, 4097, 4097) == ("t_chunked", 62, 104, 33 * 62)    # 33 tiles: ceil(2048 / 33) = 63 chunks of 102 -> 104 rows
    assert t(6400, 2047 * 128, 2047 * 128 + 1) == ("t_chunked", 2, 3200, 2 * 2047)  # 2047 tiles: ceil(2048 / 2047) = 2
    assert t(6400, 2048 * 128, 2048 * 128 + 1) == ("t_single", 1, 6400, 2048)       # 2048 tiles: one chunk
    assert t(20000, 2048) == ("t_chunked", 64, 316, 16 * 64)  # past the strip's 16384 rows


def test_the_ten_launch_forms_are_all_reachable(lib):
    """form x instantiation: the kernels tests/test_gpu_matvec.py must reach"""
    seen = set()
    for trans, rows, cols, lda in [(0, 7, 65, 66), (0, 7, 65, 65), (0, 3, 1027, 1028), (0, 3, 1027, 1027), (1, 5, 129, 130),
                                   (1, 5, 129, 129), (1, 131, 257, 258), (1, 131, 257, 257), (1, 64, 2048, 2048),
                                   (0, 5, 0, 0)]:
        d = q(lib, trans, rows, cols, lda)
        seen.add((d["form"], d["vec"]))
    assert seen == {("n_wave", 1), ("n_wave", 0), ("n_block", 1), ("n_block", 0), ("t_single", 1), ("t_single", 0),
                    ("t_chunked", 1), ("t_chunked", 0), ("t_strip", 1), ("scale", 0)}
