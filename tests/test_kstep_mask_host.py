"""Host-side checks of the weight gradient's 16-row step mask (no GPU): ia_kstep_mask_host -- the per-step function the device kernel
runs too -- against a numpy OR-reduce at 16 rows, its pairs of bits against the 32-row block mask, the size query, and the walk query of
ia_gemm_wgrad_steps on both sides of the step walk's slab-length limit."""
import numpy as np
import pytest

STEP = 16
ROWS = [1, 7, 15, 16, 17, 31, 32, 33, 16 * 77 + 1, 1275, 4080, 5389, 2048 + 17, 2048 * 16, 130560, 2048 * 64 + 100]


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
        yield density, live


@pytest.mark.parametrize("rows", ROWS)
def test_kstep_mask_host_matches_numpy(rows):
    from item_alignment_amd import _lib
    lib = _lib.load()
    for density, live in cases(rows):
        assert lib.ia_kstep_mask_bytes(rows) == 4 * ((((rows + STEP - 1) // STEP) + 31) // 32)
        got = np.full(lib.ia_kstep_mask_bytes(rows) // 4, 0xDEADBEEF, np.uint32)
        assert lib.ia_kstep_mask_host(live.ctypes.data, rows, got.ctypes.data) == 0
        assert np.array_equal(got, numpy_mask(live, STEP)), (rows, density)


@pytest.mark.parametrize("rows", ROWS)
def test_adjacent_step_bits_or_to_the_block_mask(rows):
    """what a launch with too long a k-slab folds its step mask into"""
    from item_alignment_amd import _lib
    lib = _lib.load()
    for density, live in cases(rows):
        stp = np.zeros(lib.ia_kstep_mask_bytes(rows) // 4, np.uint32)
        blk = np.zeros(lib.ia_kblock_mask_bytes(rows) // 4, np.uint32)
        assert lib.ia_kstep_mask_host(live.ctypes.data, rows, stp.ctypes.data) == 0
        assert lib.ia_kblock_mask_host(live.ctypes.data, rows, blk.ctypes.data) == 0
        bits = np.unpackbits(stp.view(np.uint8), bitorder="little")
        bits = np.concatenate([bits, np.zeros(-len(bits) % 64, np.uint8)])
        want = np.packbits(bits[0::2] | bits[1::2], bitorder="little").view(np.uint32)[: len(blk)]
        assert np.array_equal(want, blk), (rows, density)


def test_kstep_mask_argument_checks():
    from item_alignment_amd import _lib
    lib = _lib.load()
    one = np.ones(4, np.uint32)
    assert lib.ia_kstep_mask_bytes(0) == 0 and lib.ia_kstep_mask_bytes(-5) == 0
    assert lib.ia_kstep_mask_host(None, 10, one.ctypes.data) == -1
    assert lib.ia_kstep_mask_host(one.ctypes.data, 10, None) == -1
    assert lib.ia_kstep_mask_host(one.ctypes.data, 0, one.ctypes.data) == -1
    assert lib.ia_kstep_mask(None, 10, None, None) == -1


def test_wgrad_walk_query():
    """One mask word per lane is 2048 step bits: k-slabs of up to 512 k-tiles walk steps, up to 1024 blocks, longer ones every row.
    1024x1024: the plan cuts k into 16 slabs.  Host only: the query allocates and launches nothing."""
    from item_alignment_amd import _lib
    lib = _lib.load()
    # the text towers' shapes at the benchmark's 130 560 rows: 510 / 510 / 408 / 128 k-tiles per slab
    for n_out, n_in in [(1024, 4096), (4096, 1024), (3072, 1024), (1024, 1024)]:
        assert lib.ia_gemm_wgrad_walk(n_out, n_in, 130560) == 2
    assert lib.ia_gemm_wgrad_walk(1024, 1024, 512 * 64 * 16) == 2
    assert lib.ia_gemm_wgrad_walk(1024, 1024, 513 * 64 * 16) == 1
    assert lib.ia_gemm_wgrad_walk(1024, 1024, 1044480) == 1
    assert lib.ia_gemm_wgrad_walk(1024, 1024, 2088960) == 0
    assert lib.ia_gemm_wgrad_walk(4096, 4096, 32845) == 1            # 256 tiles: one slab of 514 k-tiles
    assert lib.ia_gemm_wgrad_walk(256, 256, 1275) == 0 and lib.ia_gemm_wgrad_walk(0, 8, 8) == 0
