"""Host-side checks of the row-filtered weight gradient (no GPU): the 32-row block mask as ia_kblock_mask_host computes it -- the
per-block function the device kernel runs too -- against a numpy OR-reduce at 32 rows and, pairwise, at 64 (a 64-row k-tile is live when
either of its two blocks is), the size query, and the workspace and filter queries of ia_gemm_wgrad_rows."""
import ctypes as C

import numpy as np
import pytest

BLK = 32
ROWS = [1, 31, 32, 33, 63, 64, 65, 1275, 4080, 2048 + 17, 2048 * 64, 130560, 2048 * 64 + 100]


def numpy_mask(live, step):
    n = (len(live) + step - 1) // step
    bits = np.array([live[t * step: (t + 1) * step].any() for t in range(n)] + [False] * (-n % 32))
    return (bits.reshape(-1, 32) * (1 << np.arange(32, dtype=np.uint64))).sum(1).astype(np.uint32)


def cases(rows):
    """row_live arrays behind an unaligned pointer, with live bytes behind the end that must not count"""
    rs = np.random.RandomState(rows)
    for density in (0.0, 0.002, 0.03, 0.5, 1.0):
        buf = np.zeros(rows + 3 + 64, np.uint8)
        buf[3 + rows:] = 1
        live = buf[3: 3 + rows]
        live[:] = rs.rand(rows) < density
        assert live.ctypes.data % 8 != 0      # (numpy aligns the buffer: the view starts 3 bytes in)
        yield density, live


@pytest.mark.parametrize("rows", ROWS)
def test_kblock_mask_host_matches_numpy(rows):
    from item_alignment_amd import _lib
    lib = _lib.load()
    for density, live in cases(rows):
        assert lib.ia_kblock_mask_bytes(rows) == 4 * ((((rows + BLK - 1) // BLK) + 31) // 32)
        got = np.full(lib.ia_kblock_mask_bytes(rows) // 4, 0xDEADBEEF, np.uint32)
        assert lib.ia_kblock_mask_host(live.ctypes.data, rows, got.ctypes.data) == 0
        assert np.array_equal(got, numpy_mask(live, BLK)), (rows, density)


@pytest.mark.parametrize("rows", ROWS)
def test_adjacent_block_bits_or_to_the_64_row_mask(rows):
    from item_alignment_amd import _lib
    lib = _lib.load()
    for density, live in cases(rows):
        blk = np.zeros(lib.ia_kblock_mask_bytes(rows) // 4, np.uint32)
        kt = numpy_mask(live, 2 * BLK)                      # one bit per 64-row k-tile, straight from row_live
        assert lib.ia_kblock_mask_host(live.ctypes.data, rows, blk.ctypes.data) == 0
        bits = np.unpackbits(blk.view(np.uint8), bitorder="little")
        bits = np.concatenate([bits, np.zeros(-len(bits) % 64, np.uint8)])
        pairs = bits[0::2] | bits[1::2]
        want = np.packbits(pairs, bitorder="little").view(np.uint32)[: len(kt)]
        assert np.array_equal(want, kt), (rows, density)


def test_kblock_mask_argument_checks():
    from item_alignment_amd import _lib
    lib = _lib.load()
    one = np.ones(4, np.uint32)
    assert lib.ia_kblock_mask_bytes(0) == 0 and lib.ia_kblock_mask_bytes(-5) == 0
    assert lib.ia_kblock_mask_host(None, 10, one.ctypes.data) == -1
    assert lib.ia_kblock_mask_host(one.ctypes.data, 10, None) == -1
    assert lib.ia_kblock_mask_host(one.ctypes.data, 0, one.ctypes.data) == -1
    assert lib.ia_kblock_mask(None, 10, None, None) == -1


def test_wgrad_rows_workspace_query():
    """split-K partials (rounded up to 256 bytes) in front, the block mask behind them"""
    from item_alignment_amd import _lib
    lib = _lib.load()
    al = lambda b: (b + 255) // 256 * 256
    for n_out, n_in, rows in [(1024, 1024, 130560), (4096, 1024, 130560), (3072, 1024, 32640), (256, 256, 1275), (128, 64, 70)]:
        want = al(lib.ia_gemm_workspace_bytes(n_out, n_in, rows, 1)) + lib.ia_kblock_mask_bytes(rows)
        assert lib.ia_gemm_wgrad_rows_workspace_bytes(n_out, n_in, rows) == want
    assert lib.ia_gemm_wgrad_rows_workspace_bytes(0, 8, 8) == 0
    # the text towers' weight gradients are filtered, outputs below the 256-wide kernel's plan are not
    assert lib.ia_gemm_wgrad_rows_filters(1024, 1024, 130560) == 1 and lib.ia_gemm_wgrad_rows_filters(4096, 1024, 130560) == 1
    assert lib.ia_gemm_wgrad_rows_filters(256, 256, 1275) == 0 and lib.ia_gemm_wgrad_rows_filters(0, 8, 8) == 0
    # a row filter without the workspace for its bitmask is refused before anything is launched
    buf = C.create_string_buffer(64)
    p = C.addressof(buf)
    assert lib.ia_gemm_wgrad_rows(p, 256, p, 256, p, 256, 256, 256, 1275, p, 0, None, 0, None) == -3


def test_wgrad_rows_filters_at_the_slab_length_limit():
    """The query answers for the kernel that is there: one mask word per lane is 2048 block bits, so a k-slab of more than 1024 k-tiles
    runs every row.  1024x1024: the plan cuts k into 16 slabs -- 1 044 480 rows are slabs of 1020 k-tiles (filtered), 2 088 960 rows
    slabs of 2040 (dense).  Host only: the query allocates and launches nothing."""
    from item_alignment_amd import _lib
    lib = _lib.load()
    assert lib.ia_gemm_wgrad_rows_filters(1024, 1024, 1044480) == 1
    assert lib.ia_gemm_wgrad_rows_filters(1024, 1024, 2088960) == 0
