"""ABI 20 on the host: the group-aligned list (ia_row_groups_host, the host twin of the device builder) against a Python restatement,
the layout of ia_layer_cfg in _lib.py against the header, and the new entry points among the library's symbols.

Masks: row 0 of each sequence at the two shapes the GPU tests use (24 x 577 and 41 x 255), no live row, every row live, and an M that
is no multiple of 128 (nor of 32) with live rows in its last, partial group."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from item_alignment_amd import _lib

HDR = 8      # list header words (ia_row_blocks)


def cls_mask(B, L):
    m = np.zeros(B * L, np.uint8)
    m[::L] = 1
    return m


def expected_groups(mask):
    M = mask.size
    nb = (M + 31) // 32
    live_grp = [bool(mask[g * 128: (g + 1) * 128].any()) for g in range((M + 127) // 128)]
    live = [t for t in range(nb) if live_grp[t // 4]]
    dead = [t for t in range(nb) if not live_grp[t // 4]]
    return nb, live, dead


def tail_mask():
    m = np.zeros(128 * 5 + 41, np.uint8)      # 681 rows: five whole groups and a sixth of 41 rows (two blocks, the second partial)
    m[130] = 1
    m[-1] = 1
    return m


MASKS = {"vit_cls": cls_mask(24, 577), "text_cls": cls_mask(41, 255), "empty": np.zeros(1000, np.uint8), "full": np.ones(1000, np.uint8),
         "tail": tail_mask()}


@pytest.mark.parametrize("name", sorted(MASKS))
def test_row_groups_host_matches_restatement(name):
    lib = _lib.load()
    mask = np.ascontiguousarray(MASKS[name])
    M = mask.size
    assert lib.ia_row_groups_bytes(M) == lib.ia_row_blocks_bytes(M)
    out = np.full(lib.ia_row_groups_bytes(M) // 4, -7, np.int32)
    assert lib.ia_row_groups_host(mask.ctypes.data, M, out.ctypes.data) == 0
    nb, live, dead = expected_groups(mask)
    nbr = (nb + 7) & ~7
    assert list(out[:HDR]) == [len(live), len(dead), nb, 0, 0, 0, 0, 0]
    assert list(out[HDR: HDR + len(live)]) == live
    assert list(out[HDR + nbr: HDR + nbr + len(dead)]) == dead
    # what the kernel relies on: a wave's four slots are the four blocks of one group, in order (only the last group may be short)
    for i in range(0, len(live), 4):
        run = live[i: i + 4]
        assert run[0] % 4 == 0 and run == list(range(run[0], run[0] + len(run)))
        assert len(run) == 4 or run[-1] == nb - 1


def test_row_groups_of_a_mask_without_dead_groups_is_the_block_list_of_ones():
    lib = _lib.load()
    mask = np.ascontiguousarray(MASKS["tail"])
    M = mask.size
    dil = np.zeros_like(mask)
    for g in range((M + 127) // 128):
        dil[g * 128: (g + 1) * 128] = mask[g * 128: (g + 1) * 128].any()
    a = np.zeros(lib.ia_row_groups_bytes(M) // 4, np.int32)
    b = np.zeros_like(a)
    assert lib.ia_row_groups_host(mask.ctypes.data, M, a.ctypes.data) == 0
    assert lib.ia_row_blocks_host(np.ascontiguousarray(dil).ctypes.data, M, b.ctypes.data) == 0
    nb = (M + 31) // 32
    nbr = (nb + 7) & ~7
    assert list(a[:HDR + a[0]]) == list(b[:HDR + b[0]])
    assert list(a[HDR + nbr: HDR + nbr + a[1]]) == list(b[HDR + nbr: HDR + nbr + b[1]])


def test_row_groups_rejects_bad_arguments():
    lib = _lib.load()
    out = np.zeros(64, np.int32)
    assert lib.ia_row_groups_host(None, 10, out.ctypes.data) != 0
    assert lib.ia_row_groups_host(out.ctypes.data, 0, out.ctypes.data) != 0
    assert lib.ia_row_groups_bytes(0) == 0


def header_text():
    return open(os.path.join(os.path.dirname(_lib._HERE), "include", "itemalign.h")).read()


def member_names(header, first, struct):
    body = re.search(r"typedef struct \{(\s*%s.*?)\} %s;" % (re.escape(first), struct), header, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = []
    for decl in re.findall(r"([^;]+);", body):
        for part in decl.split(","):
            names.append(re.findall(r"[A-Za-z_][A-Za-z_0-9]*", part)[-1])
    return names


def test_layer_cfg_layout_is_abi_21():
    lib = _lib.load()
    header = header_text()
    # (the layout is ABI 21's; ABI 22 took entry points away and left the struct alone)
    assert _lib.ABI_VERSION == 22 == lib.ia_abi_version() == int(re.search(r"#define IA_ABI_VERSION (\d+)", header).group(1))
    names = member_names(header, "int B, L, H, I, nh;", "ia_layer_cfg")
    assert names == [n for n, _ in _lib.LayerCfg._fields_]
    assert names[-4:] == ["masked_rows_dead", "key_rows", "out_row_live", "out_rows"]
    lists = member_names(header, "const int* blocks;", "ia_row_lists")
    assert lists == [n for n, _ in _lib.RowLists._fields_] == ["blocks", "packed", "slabs", "groups", "kblocks"]
    assert (_lib.ROWS_DEAD_BWD, _lib.ROWS_DEAD_FWD) == tuple(int(re.search(r"#define IA_ROWS_DEAD_%s (\d+)" % n, header).group(1)) for n in ("BWD", "FWD")) == (1, 2)
    # five pointers a list struct, each on its own; the two structs and out_row_live between them pointer-aligned, nothing behind them
    f, r = _lib.LayerCfg, _lib.RowLists
    assert [getattr(r, n).offset for n in lists] == [0, 8, 16, 24, 32] and C.sizeof(r) == 40
    assert f.key_rows.offset == f.masked_rows_dead.offset + 4 and f.key_rows.offset % 8 == 0
    assert f.out_row_live.offset == f.key_rows.offset + 40 and f.out_rows.offset == f.out_row_live.offset + 8
    assert C.sizeof(f) == f.out_rows.offset + 40
    c = f()
    assert c.out_row_live is None and all(getattr(rows, n) is None for rows in (c.key_rows, c.out_rows) for n in lists)
    # a member of the ABI 20 layout is no attribute: setting one raises instead of being kept where the library never looks
    for stale, obj in (("row_blocks", c), ("live_ktiles", c), ("out_row_groups", c), ("ktiles", c.key_rows)):
        with pytest.raises(AttributeError):
            setattr(obj, stale, 256)


def test_new_entry_points_are_declared_bound_and_exported():
    lib = _lib.load()
    header = header_text()
    for name in ("ia_row_groups_bytes", "ia_row_groups", "ia_row_groups_host", "ia_gemm_fwd_rows_add", "ia_gemm_dgrad_groups_rows",
                 "ia_debug_out_rows"):
        assert re.search(r"\b%s\(" % name, header), name
        assert name in _lib.SIGNATURES, name
        assert getattr(lib, name) is not None, name
    was = lib.ia_debug_out_rows(0)
    assert was == 1 and lib.ia_debug_out_rows(1) == 0 and lib.ia_debug_out_rows(was) == 1
