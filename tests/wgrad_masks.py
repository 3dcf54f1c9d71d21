"""Row masks of the row-filtered weight-gradient tests (ia_gemm_wgrad_rows, ia_gemm_wgrad_blocks), the k-slab plan they are laid out against,
and the error measure both files use.

A k-tile is 64 rows of k (one trip of the dense kernel's loop), a k-slab the run of k-tiles one split-K workgroup owns; the filtered kernel
walks the live 32-row blocks of its slab, two to a trip."""
import numpy as np

BK = 64


def rel_err(a, b):
    a, b = a.double(), b.double()
    return ((a - b).abs().max() / (b.abs().max() + 1e-12)).item()


def slab_tiles(n_out, n_in, rows):
    """k-tiles per k-slab of the plan both entry points use"""
    from item_alignment_amd import _lib
    lib = _lib.load()
    nk = (rows + BK - 1) // BK
    splits = max(1, lib.ia_gemm_workspace_bytes(n_out, n_in, rows, 1) // (n_out * (n_in + 1) * 4))
    return nk, (nk + splits - 1) // splits


def patterns(n_out, n_in, rows):
    """name -> row_live (numpy uint8 [rows])"""
    nk, per = slab_tiles(n_out, n_in, rows)
    tile = lambda t: slice(t * BK, min(rows, (t + 1) * BK))
    out = {"all_live": np.ones(rows, np.uint8), "all_dead": np.zeros(rows, np.uint8)}
    # right-padded sequences of 255 positions, lengths 3 + U[8,48] + U[16,203] as the benchmark's synthetic data draws them
    rs = np.random.RandomState(2345)
    L = 255
    live = np.zeros((rows + L - 1) // L * L, np.uint8)
    for b in range(len(live) // L):
        live[b * L: b * L + 3 + rs.randint(8, 49) + rs.randint(16, 204)] = 1
    out["padded"] = live[:rows].copy()
    s = np.ones(rows, np.uint8)          # one slab dead (the second if there is one), its neighbours live
    first = per if nk > per else 0
    s[first * BK: min(rows, (first + per) * BK)] = 0
    out["slab_dead"] = s
    e = np.ones(rows, np.uint8)          # first and last k-tile of every slab dead
    for t0 in range(0, nk, per):
        e[tile(t0)] = 0
        e[tile(min(nk, t0 + per) - 1)] = 0
    out["slab_edges_dead"] = e
    t = np.ones(rows, np.uint8); t[tile(nk - 1)] = 0
    out["tail_dead"] = t
    t = np.zeros(rows, np.uint8); t[tile(nk - 1)] = 1; t[tile(0)] = 1
    out["tail_live"] = t
    o = np.zeros(rows, np.uint8); o[rows // 2 + 7] = 1
    out["one_row"] = o
    return out
