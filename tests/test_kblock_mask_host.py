"""Host-side checks of the 32-row block mask (no GPU): ia_kblock_mask_host -- the per-block function the device kernel runs too -- against a
numpy OR-reduce, against ia_ktile_mask_host (a 64-row k-tile is live when either of its two blocks is), and the size query."""
import numpy as np
import pytest

BLK = 32
ROWS = [1, 31, 32, 33, 1275, 4080, 130560]


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
def test_adjacent_block_bits_or_to_the_ktile_mask(rows):
    from item_alignment_amd import _lib
    lib = _lib.load()
    for density, live in cases(rows):
        blk = np.zeros(lib.ia_kblock_mask_bytes(rows) // 4, np.uint32)
        kt = np.zeros(lib.ia_ktile_mask_bytes(rows) // 4, np.uint32)
        assert lib.ia_kblock_mask_host(live.ctypes.data, rows, blk.ctypes.data) == 0
        assert lib.ia_ktile_mask_host(live.ctypes.data, rows, kt.ctypes.data) == 0
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
