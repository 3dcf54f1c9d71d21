"""The 8-row slab list on the host: ia_row_slabs_host (the host twin of the device builder) against the numpy restatement of
tests/slab_masks.py, the header counts, the [tile][wave][piece] order, and the new entry points among the library's symbols.

Masks: every row live, none, one row, every other slab, a live row only in the partial last slab, fewer than / exactly / more than one
tile of slabs, tiles that leave a wave without a slab, and lengths drawn as data/synthetic.py draws them at L = 255 -- at M = 264 (33
slabs), 765 (= 3 x 255: the last slab holds 5 rows) and 1032, the row counts of the GPU tests, and at 41 x 255."""
import os
import re

import numpy as np
import pytest

from item_alignment_amd import _lib

from slab_masks import HDR, TILE, expected_list, expected_slabs, named_masks, slot

CASES = [(M, name) for M in (264, 765, 1032, 41 * 255) for name in sorted(named_masks(M))]


def build(lib, mask):
    mask = np.ascontiguousarray(mask)
    out = np.full(lib.ia_row_slabs_bytes(mask.size) // 4, -7, np.int32)
    assert lib.ia_row_slabs_host(mask.ctypes.data, mask.size, out.ctypes.data) == 0
    return out


@pytest.mark.parametrize("M,name", CASES)
def test_row_slabs_host_matches_restatement(M, name):
    lib = _lib.load()
    mask = named_masks(M)[name]
    ns = (M + 7) // 8
    nsr = (ns + TILE - 1) // TILE * TILE
    assert lib.ia_row_slabs_bytes(M) == (HDR + 2 * nsr) * 4
    out = build(lib, mask)
    want = expected_list(mask)
    assert len(want) == out.size
    for i, w in enumerate(want):
        assert out[i] == (w if w is not None else -7), (i, w, out[i])      # (-7: a word the builder has no business writing)


@pytest.mark.parametrize("M,name", CASES)
def test_header_counts_and_tile_order(M, name):
    lib = _lib.load()
    mask = named_masks(M)[name]
    out = build(lib, mask)
    ns, live, dead = expected_slabs(mask)
    assert list(out[:HDR]) == [len(live), len(dead), ns, 0, 0, 0, 0, 0] and len(live) + len(dead) == ns
    # reading a tile back the way the kernel addresses it: wave w's eight DMA entries are one aligned run of 8 words, piece j of it is
    # slab 4j + w of the tile; in that order the tile's slabs ascend, and so do the tiles
    got = []
    for tile in range((len(live) + TILE - 1) // TILE):
        words = out[HDR + tile * TILE: HDR + (tile + 1) * TILE].reshape(4, 8)      # [wave][piece]
        asc = [int(words[t & 3, t >> 2]) for t in range(TILE)]
        n = min(TILE, len(live) - tile * TILE)
        assert all(v == -1 for v in asc[n:])
        # the epilogue's view: wave-row wm, block mi, pass it -> entry it * 8 + wm * 4 + mi is row 32 (4 wm + mi) + 8 it of the tile
        for wm in range(2):
            for mi in range(4):
                for it in range(4):
                    assert out[HDR + tile * TILE + it * 8 + wm * 4 + mi] == asc[(wm * 4 + mi) * 4 + it]
        got += asc[:n]
    assert got == live == sorted(live)
    assert all(slot(i) == (i // TILE) * TILE + (i % 4) * 8 + (i % TILE) // 4 for i in range(3 * TILE))
    # the last slab is partial when 8 does not divide M: it is listed like any other, live or dead
    if M % 8:
        assert (ns - 1 in live) == bool(mask[8 * (ns - 1):].any())


def test_device_and_host_lists_share_one_offset_rule():
    """(no offset rule is left: a list has a pointer of its own in ia_row_lists; the slab entries' workspace is the list and nothing else)"""
    lib = _lib.load()
    for M in (264, 765, 130560):
        assert lib.ia_gemm_slabs_workspace_bytes(M) == lib.ia_row_slabs_bytes(M)


def test_row_slabs_rejects_bad_arguments():
    lib = _lib.load()
    out = np.zeros(128, np.int32)
    assert lib.ia_row_slabs_host(None, 10, out.ctypes.data) != 0
    assert lib.ia_row_slabs_host(out.ctypes.data, 0, out.ctypes.data) != 0
    assert lib.ia_row_slabs_bytes(0) == 0


def test_slab_entry_points_are_declared_bound_and_exported():
    lib = _lib.load()
    header = open(os.path.join(os.path.dirname(_lib._HERE), "include", "itemalign.h")).read()
    assert _lib.ABI_VERSION == 22 == lib.ia_abi_version() == int(re.search(r"#define IA_ABI_VERSION (\d+)", header).group(1))
    for name in ("ia_row_slabs_bytes", "ia_row_slabs", "ia_row_slabs_host", "ia_gemm_slabs_workspace_bytes",
                 "ia_gemm_fwd_slabs", "ia_gemm_dgrad_slabs"):
        assert re.search(r"\b%s\(" % name, header), name
        assert name in _lib.SIGNATURES, name
        assert getattr(lib, name) is not None, name
