"""Row masks and the numpy restatement of the 8-row slab list (ia_row_slabs), shared by the host test of the builder and the GPU tests of
the slab GEMMs.

A slab is rows 8t .. 8t+7 of the tensor, clipped to M; it is live when one of its rows is.  The list: 8 header words (live, dead, slabs),
the live slabs ascending with the i-th at entry slot(i) -- 32 to an M-tile, [wave][piece] inside a tile -- and -1 behind the last of the
last tile; the dead slabs, ascending, behind room for every slab rounded up to a multiple of 32."""
import numpy as np

HDR = 8
TILE = 32


def slot(i):
    return (i & ~31) + (i & 3) * 8 + ((i & 31) >> 2)


def expected_slabs(mask):
    M = mask.size
    ns = (M + 7) // 8
    flags = [bool(mask[8 * t: 8 * t + 8].any()) for t in range(ns)]
    live = [t for t in range(ns) if flags[t]]
    dead = [t for t in range(ns) if not flags[t]]
    return ns, live, dead


def expected_list(mask):
    """the whole list as int32 words, None where the builder leaves a word unwritten"""
    ns, live, dead = expected_slabs(mask)
    nsr = (ns + TILE - 1) // TILE * TILE
    out = [None] * (HDR + 2 * nsr)
    out[:HDR] = [len(live), len(dead), ns, 0, 0, 0, 0, 0]
    for i, t in enumerate(live):
        out[HDR + slot(i)] = t
    for i in range(len(live), (len(live) + TILE - 1) // TILE * TILE):
        out[HDR + slot(i)] = -1
    for i, t in enumerate(dead):
        out[HDR + nsr + i] = t
    return out


def slab_dilate(mask):
    """row mask of the rows the slab form computes: every row of a slab that holds a live row"""
    out = np.zeros_like(mask)
    for t in range((mask.size + 7) // 8):
        out[8 * t: 8 * t + 8] = mask[8 * t: 8 * t + 8].any()
    return out


def lengths_mask(B, L, seed, lengths=None):
    """B sequences of L positions, the first len_b live: lengths drawn as data/synthetic.py draws them (3 + U{8..48} + U{16..203},
    clipped to L), or given"""
    rs = np.random.RandomState(seed)
    m = np.zeros((B, L), np.uint8)
    for b in range(B):
        n = lengths[b] if lengths is not None else min(L, 3 + int(rs.randint(8, 49)) + int(rs.randint(16, 204)))
        m[b, :n] = 1
    return m.reshape(-1)


def one_row(M, r):
    m = np.zeros(M, np.uint8)
    m[r] = 1
    return m


def alternating(M):
    m = np.zeros(M, np.uint8)
    for t in range(0, (M + 7) // 8, 2):
        m[8 * t + 3: 8 * t + 4] = 1      # one live row in every other slab
    return m


def first_slabs(M, n):
    """one live row in each of the first n slabs of M rows (n < 32: one short tile; 32: exactly one; 33: one and a slab).  Wave w of a
    tile carries its slabs 4j + w: a tile of fewer than four slabs (n = 3, n = 35) leaves a wave without one."""
    m = np.zeros(M, np.uint8)
    for i in range(n):
        m[min(M - 1, 8 * i + (i % 8))] = 1
    return m


def named_masks(M):
    """the masks of the host test at M rows (M = 255 * k for the drawn lengths; any M for the others)"""
    out = {
        "all": np.ones(M, np.uint8),
        "none": np.zeros(M, np.uint8),
        "one_row": one_row(M, min(M - 1, 77)),
        "alternating": alternating(M),
        "last_partial": one_row(M, M - 1),
        "short_tile": first_slabs(M, 20),
        "one_tile": first_slabs(M, 32),
        "tile_and_one": first_slabs(M, 33),
        "wave_without_slab": first_slabs(M, 3),
    }
    if M > 8 * 34:
        out["tile_and_wave_without_slab"] = first_slabs(M, 35)
    if M % 255 == 0:
        out["lengths"] = lengths_mask(M // 255, 255, seed=M)
    return out
