"""Host-side checks of the row-filtered weight gradient (no GPU): the live-k-tile bitmask as ia_ktile_mask_host computes it -- the
per-k-tile function the device kernel runs too -- against a numpy OR-reduce, and the workspace query of ia_gemm_wgrad_rows."""
import ctypes as C

import numpy as np
import pytest

BK = 64


def numpy_mask(live):
    nk = (len(live) + BK - 1) // BK
    bits = np.array([live[t * BK: (t + 1) * BK].any() for t in range(nk)] + [False] * (-nk % 32))
    return (bits.reshape(-1, 32) * (1 << np.arange(32, dtype=np.uint64))).sum(1).astype(np.uint32)


@pytest.mark.parametrize("rows", [1, 63, 64, 65, 1275, 4080, 2048 + 17, 2048 * 64, 130560, 2048 * 64 + 100])
@pytest.mark.parametrize("offset", [0, 3])
def test_ktile_mask_host_matches_numpy(rows, offset):
    from item_alignment_amd import _lib
    lib = _lib.load()
    rs = np.random.RandomState(rows)
    for density in (0.0, 0.002, 0.5, 1.0):
        buf = np.zeros(rows + offset + 64, np.uint8)
        buf[offset + rows:] = 1                                   # rows behind the end must not count
        live = buf[offset: offset + rows]
        live[:] = rs.rand(rows) < density
        assert lib.ia_ktile_mask_bytes(rows) == 4 * ((((rows + BK - 1) // BK) + 31) // 32)
        got = np.full(lib.ia_ktile_mask_bytes(rows) // 4, 0xDEADBEEF, np.uint32)
        assert lib.ia_ktile_mask_host(live.ctypes.data, rows, got.ctypes.data) == 0
        assert np.array_equal(got, numpy_mask(live)), (rows, offset, density)


def test_ktile_mask_argument_checks():
    from item_alignment_amd import _lib
    lib = _lib.load()
    one = np.ones(4, np.uint32)
    assert lib.ia_ktile_mask_bytes(0) == 0 and lib.ia_ktile_mask_bytes(-5) == 0
    assert lib.ia_ktile_mask_host(None, 10, one.ctypes.data) == -1
    assert lib.ia_ktile_mask_host(one.ctypes.data, 0, one.ctypes.data) == -1
    assert lib.ia_ktile_mask(None, 10, None, None) == -1


def test_wgrad_rows_workspace_query():
    """split-K partials (rounded up to 256 bytes) in front, the bitmask behind them"""
    from item_alignment_amd import _lib
    lib = _lib.load()
    al = lambda b: (b + 255) // 256 * 256
    for n_out, n_in, rows in [(1024, 1024, 130560), (4096, 1024, 130560), (3072, 1024, 32640), (256, 256, 1275), (128, 64, 70)]:
        want = al(lib.ia_gemm_workspace_bytes(n_out, n_in, rows, 1)) + lib.ia_ktile_mask_bytes(rows)
        assert lib.ia_gemm_wgrad_rows_workspace_bytes(n_out, n_in, rows) == want
    assert lib.ia_gemm_wgrad_rows_workspace_bytes(0, 8, 8) == 0
    # the text towers' weight gradients are filtered, outputs below the 256-wide kernel's plan are not
    assert lib.ia_gemm_wgrad_rows_filters(1024, 1024, 130560) == 1 and lib.ia_gemm_wgrad_rows_filters(4096, 1024, 130560) == 1
    assert lib.ia_gemm_wgrad_rows_filters(256, 256, 1275) == 0 and lib.ia_gemm_wgrad_rows_filters(0, 8, 8) == 0
    # a row filter without the workspace for its bitmask is refused before anything is launched
    buf = C.create_string_buffer(64)
    p = C.addressof(buf)
    assert lib.ia_gemm_wgrad_rows(p, 256, p, 256, p, 256, 256, 256, 1275, p, 0, None, 0, None) == -3
