"""Host-side checks of the row-filtered data gradient (no GPU): the 32-row block list as ia_row_blocks_host computes it -- through the
per-block function the device kernel runs too -- against numpy, and the workspace / filter queries of ia_gemm_dgrad_rows."""
import ctypes as C

import numpy as np
import pytest

BLK, HDR = 32, 8


def numpy_lists(live):
    nb = (len(live) + BLK - 1) // BLK
    any_live = np.array([live[t * BLK: (t + 1) * BLK].any() for t in range(nb)], bool)
    idx = np.arange(nb, dtype=np.int32)
    return nb, idx[any_live], idx[~any_live]


def check_list(got, live):
    nb, want_live, want_dead = numpy_lists(live)
    nbr = (nb + 7) // 8 * 8
    assert len(got) == HDR + 2 * nbr
    assert list(got[:HDR]) == [len(want_live), len(want_dead), nb, 0, 0, 0, 0, 0]
    assert np.array_equal(got[HDR: HDR + len(want_live)], want_live)
    assert np.array_equal(got[HDR + nbr: HDR + nbr + len(want_dead)], want_dead)


def host_list(lib, live):
    rows = len(live)
    assert lib.ia_row_blocks_bytes(rows) == 4 * (HDR + 2 * ((((rows + BLK - 1) // BLK) + 7) // 8 * 8))
    got = np.full(lib.ia_row_blocks_bytes(rows) // 4, -559038737, np.int32)
    assert lib.ia_row_blocks_host(live.ctypes.data, rows, got.ctypes.data) == 0
    return got


def cases(rows):
    """name -> row_live (uint8 [rows])"""
    nb = (rows + BLK - 1) // BLK
    out = {"all_live": np.ones(rows, np.uint8), "all_dead": np.zeros(rows, np.uint8)}
    alt = np.zeros(rows, np.uint8)
    for t in range(0, nb, 2):
        alt[t * BLK: (t + 1) * BLK] = 1
    out["alternating"] = alt
    out["alternating_odd"] = 1 - alt
    for name, pos in (("first_of_block", (nb // 2) * BLK), ("last_of_block", min(rows, (nb // 2 + 1) * BLK) - 1), ("row_0", 0), ("last_row", rows - 1)):
        one = np.zeros(rows, np.uint8)
        one[pos] = 1
        out["single_" + name] = one
    tail_live = np.zeros(rows, np.uint8); tail_live[(nb - 1) * BLK:] = 1       # the last block (partial unless rows is a multiple of 32) alone
    out["last_block_live"] = tail_live
    out["last_block_dead"] = 1 - tail_live
    rs = np.random.RandomState(rows)
    out["random_sparse"] = (rs.rand(rows) < 0.01).astype(np.uint8)
    return out


@pytest.mark.parametrize("rows", [1, 31, 32, 33, 8159, 5100, 130560])
@pytest.mark.parametrize("offset", [0, 3])
def test_row_blocks_host_matches_numpy(rows, offset):
    from item_alignment_amd import _lib
    lib = _lib.load()
    for name, pattern in cases(rows).items():
        buf = np.zeros(rows + offset + 64, np.uint8)
        buf[offset + rows:] = 1                                   # rows behind the end must not count
        live = buf[offset: offset + rows]
        live[:] = pattern
        check_list(host_list(lib, live), live)


def test_row_blocks_partial_last_block():
    """8159 = 254 * 32 + 31 rows: the last block holds 31 rows; live through its last row only, and dead"""
    from item_alignment_amd import _lib
    lib = _lib.load()
    live = np.zeros(8159, np.uint8)
    live[8158] = 1
    got = host_list(lib, live)
    assert got[0] == 1 and got[HDR] == 254 and got[1] == 254
    live[8158] = 0
    live[8127] = 1                                                # the last row of the block in front of it
    got = host_list(lib, live)
    assert got[0] == 1 and got[HDR] == 253 and got[HDR + 256 + 253] == 254


def test_row_blocks_argument_checks():
    from item_alignment_amd import _lib
    lib = _lib.load()
    one = np.ones(64, np.int32)
    assert lib.ia_row_blocks_bytes(0) == 0 and lib.ia_row_blocks_bytes(-5) == 0
    assert lib.ia_row_blocks_host(None, 10, one.ctypes.data) == -1
    assert lib.ia_row_blocks_host(one.ctypes.data, 0, one.ctypes.data) == -1
    assert lib.ia_row_blocks(None, 10, None, None) == -1


def test_dgrad_rows_queries():
    """column-sum partials (rounded up to 256 bytes) in front, the block list behind them; large plans filter, small ones do not"""
    from item_alignment_amd import _lib
    lib = _lib.load()
    al = lambda b: (b + 255) // 256 * 256
    for rows, n_in, k_out in [(130560, 4096, 1024), (130560, 1024, 3072), (5100, 2048, 64), (1275, 256, 256), (70, 64, 128)]:
        want = al(lib.ia_gemm_colsum_workspace_bytes(rows, n_in)) + lib.ia_row_blocks_bytes(rows)
        assert lib.ia_gemm_dgrad_rows_workspace_bytes(rows, n_in, k_out) == want
    assert lib.ia_gemm_dgrad_rows_workspace_bytes(0, 8, 8) == 0
    # the text towers' data gradients and the smallest 160-tile plan are filtered; outputs below the 256-wide kernel's plan are not
    assert lib.ia_gemm_dgrad_rows_filters(130560, 4096, 1024) == 1 and lib.ia_gemm_dgrad_rows_filters(130560, 1024, 4096) == 1
    assert lib.ia_gemm_dgrad_rows_filters(130560, 1024, 3072) == 1 and lib.ia_gemm_dgrad_rows_filters(5100, 2048, 64) == 1
    assert lib.ia_gemm_dgrad_rows_filters(1275, 256, 256) == 0 and lib.ia_gemm_dgrad_rows_filters(4845, 2048, 64) == 0
    assert lib.ia_gemm_dgrad_rows_filters(0, 8, 8) == 0
    # an operand the 32-bit buffer window of the remapped kernel cannot span runs every row
    assert lib.ia_gemm_dgrad_rows_filters(300000, 4096, 1024) == 0
    # a row filter without the workspace for its list is refused before anything is launched, and so is another epilogue
    buf = C.create_string_buffer(64)
    p = C.addressof(buf)
    assert lib.ia_gemm_dgrad_rows(p, 256, p, 1, 256, p, 256, 1275, 256, 256, 0, None, 0, None, p, None, 0, None) == -3
    assert lib.ia_gemm_dgrad_rows(p, 256, p, 1, 256, p, 256, 1275, 256, 256, 1, None, 0, None, p, None, 0, None) != 0
