"""Times the graph two-tower train step and its kernels at the reference size (N = 230 023 nodes, C = 128, L = 4, P = 512, F = 1024)
on a SyntheticItemGraph, and prints ms and achieved GB/s per kernel next to the bytes each one has to move.

    python tools/gcn_bench.py [--items 180023 --values 50000 --steps 5]

Bytes counted per kernel (fp32; an operand is counted once even where the 64-column tiles fetch it twice): propagate forward =
nnz * C * 4 gathered + 2 [N, C] (x_0 read, h written); propagate backward = nnz * C * 4 gathered + 4 [N, C] (dh read for the blend,
dx written, dx_0 read and written); mix forward = 2 [N, C] (h read, output written); mix backward = 6 [N, C] (dout, out read and dh
written for the data gradient; h, dout, out read for dW); input forward = X once + [N, C]; input backward = X once + 2 [N, C] + the
partial slabs written and read once.
"""
import argparse
import os
import sys
import time
from types import SimpleNamespace

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(reps + 1)]
    ev[0].record()
    for i in range(reps):
        fn()
        ev[i + 1].record()
    torch.cuda.synchronize()
    return sorted(ev[i].elapsed_time(ev[i + 1]) for i in range(reps))[reps // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--items", type=int, default=180023)
    ap.add_argument("--values", type=int, default=50000)
    ap.add_argument("--features", type=int, default=1024)
    ap.add_argument("--width", type=int, default=128)
    ap.add_argument("--layers", type=int, default=4)
    ap.add_argument("--pairs", type=int, default=512)
    ap.add_argument("--steps", type=int, default=5)
    a = ap.parse_args()
    from item_alignment_amd import _lib
    from item_alignment_amd.data.synthetic import SyntheticItemGraph
    from item_alignment_amd.models import GCNTwoTower, load_adjacency
    from item_alignment_amd.train import ArenaAdamW
    lib = _lib.load()
    t0 = time.time()
    g = SyntheticItemGraph(a.items, a.values, feature_dim=4, n_pairs=a.pairs)
    adj = load_adjacency(g.edge_index, num_nodes=g.num_nodes, device="cuda")
    N, C, F, L, nnz = g.num_nodes, a.width, a.features, a.layers, adj.nnz
    deg = adj.rowptr[1:] - adj.rowptr[:-1]
    print(f"graph: N = {N}, nnz = {nnz}, max degree {int(deg.max())}, rows over 512 neighbours: {adj.long_rows.numel()}  (built in {time.time() - t0:.1f} s)")
    X = torch.randn((N, F), device="cuda")
    cfg = SimpleNamespace(hidden_size=F, intermediate_size=C, num_hidden_layers=L, hidden_dropout_prob=0.1, num_labels=2, alpha=0.1, theta=0.5,
                          loss_type="ce")
    os.environ["IA_GCN_PAIRWISE_LOSS"] = "1"
    model = GCNTwoTower(cfg).cuda().train()
    opt = ArenaAdamW(model, 1e-3, 1e-8, 1e-5)
    pairs = g.pairs[:a.pairs]

    def step():
        opt.zero_grad()
        model(X, adj, pairs).loss.backward()
        opt.step(1.0)

    ms = timed(step, a.steps)
    print(f"train step (forward + backward + AdamW, dropout 0.1): {ms:.2f} ms")
    s, P_ = _lib.stream_ptr, (lambda t: None if t is None else t.data_ptr())
    nc = N * C * 4
    x, x0, h, o, d2 = (torch.randn((N, C), device="cuda") for _ in range(5))
    W = torch.randn((C, C), device="cuda") / C ** 0.5
    Wi, bi = torch.randn((C, F), device="cuda") / F ** 0.5, torch.zeros(C, device="cuda")
    dW, dWi, dbi = torch.zeros_like(W), torch.zeros_like(Wi), torch.zeros_like(bi)
    wsb = int(lib.ia_gcn_workspace_bytes(N, C, F))
    ws = torch.empty(wsb, dtype=torch.uint8, device="cuda")
    lr, lrt = adj.long_rows, adj.long_rows_t
    rows = [
        ("propagate_fwd", nnz * C * 4 + 2 * nc, lambda: lib.ia_gcn_propagate_fwd(P_(adj.rowptr), P_(adj.col), 0, P_(adj.val), P_(x), P_(x0), P_(h), N, C, 0.1,
                                                                                 0.1, 1, 3001, P_(lr) if lr.numel() else None, lr.numel(), s())),
        ("propagate_bwd", nnz * C * 4 + 4 * nc, lambda: lib.ia_gcn_propagate_bwd(P_(adj.rowptr_t), P_(adj.col_t), 0, P_(adj.val_t), P_(h), P_(o), P_(d2), 1, N,
                                                                                 C, 0.1, 0.1, 1, 3001, P_(lrt) if lrt.numel() else None, lrt.numel(), s())),
        ("mix_fwd", 2 * nc, lambda: lib.ia_gcn_mix_fwd(P_(h), P_(W), P_(o), N, C, 0.2, 0.0, 1, 3005, s())),
        ("mix_bwd", 6 * nc, lambda: lib.ia_gcn_mix_bwd(P_(x), P_(o), P_(h), P_(W), P_(d2), P_(dW), N, C, 0.2, 0.0, P_(ws), wsb, s())),
        ("input_fwd", N * F * 4 + nc, lambda: lib.ia_gcn_input_fwd(P_(X), P_(Wi), P_(bi), P_(x0), N, F, C, 0.1, 1, 3000, s())),
        ("input_bwd", N * F * 4 + 2 * nc + 2 * wsb, lambda: lib.ia_gcn_input_bwd(P_(x), P_(x0), P_(X), P_(dWi), P_(dbi), N, F, C, 0.1, 1, 3000, P_(ws), wsb, s())),
    ]
    for name, nbytes, fn in rows:
        assert fn() == 0, name
        ms = timed(fn, a.steps)
        print(f"{name:14s} {ms:8.3f} ms   {nbytes / 1e6:9.1f} MB   {nbytes / ms / 1e6:8.1f} GB/s")


if __name__ == "__main__":
    main()
