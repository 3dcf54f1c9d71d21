#!/usr/bin/env python3
"""Trips of the filtered weight gradient's busiest k-slab, by walk: whole 64-row k-tiles (dense), live 32-row blocks two to a trip, live
16-row steps four to a trip.  CPU only: the synthetic lengths of the benchmark (3 + U[8,48] + U[16,203] of 255), the k-slabs of the
library's own split-K plan.  usage: wgrad_trip_counts.py [sequences] [seeds]"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from item_alignment_amd import _lib  # noqa: E402

BK, L = 64, 255
SHAPES = [("QKV", 3072, 1024), ("fc1", 4096, 1024), ("fc2", 1024, 4096), ("out-projection", 1024, 1024)]


def live_rows(n_seq, seed):
    rs = np.random.RandomState(seed)
    live = np.zeros(n_seq * L, np.uint8)
    for b in range(n_seq):
        live[b * L: b * L + 3 + rs.randint(8, 49) + rs.randint(16, 204)] = 1
    return live


def units(live, rows):
    n = (len(live) + rows - 1) // rows
    pad = np.zeros(n * rows, np.uint8)
    pad[:len(live)] = live
    return pad.reshape(n, rows).any(axis=1)


def main():
    n_seq = int(sys.argv[1]) if len(sys.argv) > 1 else 512
    seeds = int(sys.argv[2]) if len(sys.argv) > 2 else 4
    lib = _lib.load()
    M = n_seq * L
    nk = (M + BK - 1) // BK
    shares = {16: [], 32: []}
    for name, n_out, n_in in SHAPES:
        splits = max(1, lib.ia_gemm_workspace_bytes(n_out, n_in, M, 1) // (n_out * (n_in + 1) * 4))
        per = (nk + splits - 1) // splits
        rows = []
        for seed in range(seeds):
            live = live_rows(n_seq, seed)
            blk, stp = units(live, 32), units(live, 16)
            if name == "QKV":
                shares[32].append(blk.mean()); shares[16].append(stp.mean())
            tb = max(-(-int(blk[2 * s * per: 2 * (s + 1) * per].sum()) // 2) for s in range(splits))
            ts = max(-(-int(stp[4 * s * per: 4 * (s + 1) * per].sum()) // 4) for s in range(splits))
            rows.append((tb, ts))
        tb, ts = [r[0] for r in rows], [r[1] for r in rows]
        ratio = [s / b for b, s in rows]
        print(f"{name:15s} {splits:2d} slabs of {per:3d} k-tiles (walk {lib.ia_gemm_wgrad_walk(n_out, n_in, M)}): busiest slab "
              f"{min(tb)}-{max(tb)} trips by blocks -> {min(ts)}-{max(ts)} by steps, x{min(ratio):.3f}-{max(ratio):.3f}")
    print(f"share of M: 32-row blocks {min(shares[32]):.3f}-{max(shares[32]):.3f}, 16-row steps {min(shares[16]):.3f}-{max(shares[16]):.3f}")


if __name__ == "__main__":
    main()
