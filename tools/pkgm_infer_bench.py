"""Time of knowledge-graph completion (pkgm_infer.py, ia_kgpt_topk) on one GPU at the shape of tools/pkgm_linkpred_bench.py: 258 211
entities x 768, B = 4 096 queries, the top 10 tails, L2 and L1, unfiltered and with 16-member filter groups.  In the same process, on
the same queries:
  (a) ia_kgpt_lp_rank on the tail side: the same scan without the selection -- the figure the top-k kernel is held against;
  (b) the reference's formulation in plain torch on the GPU (unfiltered): the [chunk, n_ent] score matrix by broadcast, then sort.
The kernels alternate (topk, rank, topk_filtered in one order, then the reverse) after a warm-up; the medians of the device-event
times are reported, with ratio_to_rank = topk / rank.

    python tools/pkgm_infer_bench.py [--out profiles/pkgm_infer_bench.json] [--batch 4096] [--dim 768] [--reps 7]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--n_ent", type=int, default=258211)
    ap.add_argument("--top_k", type=int, default=10)
    ap.add_argument("--norms", type=int, nargs="+", default=[2, 1])
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--baseline_queries", type=int, default=64)
    ap.add_argument("--baseline_chunk", type=int, default=4)
    args = ap.parse_args()
    import numpy as np
    import torch
    from item_alignment_amd.models import kg_pretrain as K
    if not torch.cuda.is_available():
        raise SystemExit("pkgm_infer_bench.py measures on the GPU")
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(0)
    n_ent, n_rel, B, D, k = args.n_ent, 1379, args.batch, args.dim, args.top_k
    g = torch.Generator(device=dev).manual_seed(D)
    ent = torch.randn(n_ent, D, device=dev, generator=g) * 0.05
    rel = torch.randn(n_rel, D, device=dev, generator=g) * 0.05
    h, t = (torch.randint(0, n_ent, (B,), device=dev, generator=g) for _ in range(2))
    r = torch.randint(0, n_rel, (B,), device=dev, generator=g)
    lib = K._lib.load()
    ws_rank = torch.empty(lib.ia_kgpt_lp_workspace_bytes(B, D), device=dev, dtype=torch.uint8)
    ws_topk = torch.empty(lib.ia_kgpt_topk_workspace_bytes(B, D, n_ent, k, 0), device=dev, dtype=torch.uint8)
    ids = np.sort(np.concatenate([t.cpu().numpy()[:, None], rng.integers(0, n_ent, (B, 15))], 1), 1).reshape(-1)
    groups = K._DeviceGroups(K.FilterGroups(np.arange(B, dtype=np.int64), np.arange(0, 16 * B + 1, 16, dtype=np.int64), ids, 1), dev)
    qg = torch.arange(B, device=dev)

    def timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b)

    results = []
    for norm in args.norms:
        arms = {"topk": lambda: K.kg_topk(ent, rel, h, r, norm, K.TOPK_TAILS, k, workspace=ws_topk),
                "rank": lambda: K.lp_rank(ent, rel, h, t, r, norm, K.LP_TAIL, workspace=ws_rank),
                "topk_filtered": lambda: K.kg_topk(ent, rel, h, r, norm, K.TOPK_TAILS, k, groups, qg, workspace=ws_topk)}
        for fn in arms.values():                                # warm-up: code objects, the allocator
            fn()
            fn()
        torch.cuda.synchronize()
        ms = {name: [] for name in arms}
        for rep in range(args.reps):
            order = list(arms) if rep % 2 == 0 else list(arms)[::-1]
            for name in order:
                ms[name].append(timed(arms[name]))
        med = {name: statistics.median(v) for name, v in ms.items()}
        # the selection must not have changed the answer: the unfiltered top-1 is where the stored matrix has its maximum
        idx, score = K.kg_topk(ent, rel, h[:8], r[:8], norm, K.TOPK_TAILS, k)
        sc = K.lp_rank(ent, rel, h[:8], t[:8], r[:8], norm, K.LP_TAIL, want_scores=True)[2]
        top, arg = sc.sort(dim=1, descending=True, stable=True)
        assert torch.equal(score, top[:, :k]) and torch.equal(idx, arg[:, :k])
        pairs = float(B) * n_ent * D
        row = dict(n_ent=n_ent, dim=D, norm=norm, batch=B, top_k=k, reps=args.reps,
                   topk_ms=round(med["topk"], 2), rank_ms=round(med["rank"], 2), topk_filtered_ms=round(med["topk_filtered"], 2),
                   ratio_to_rank=round(med["topk"] / med["rank"], 3), filtered_ratio_to_rank=round(med["topk_filtered"] / med["rank"], 3),
                   topk_pairs_per_s=float(f"{pairs / (med['topk'] * 1e-3):.4g}"),
                   spread_ms={name: [round(min(v), 2), round(max(v), 2)] for name, v in ms.items()},
                   workspace_bytes=ws_topk.numel(), matrix_bytes=4 * B * n_ent)
        results.append(row)
        print(json.dumps(row), flush=True)
    # (b) the reference's formulation in plain torch (L2): scores by broadcast in query chunks, then a full sort
    nq, ch = args.baseline_queries, args.baseline_chunk

    def reference():
        for i in range(0, nq, ch):
            s = -((ent[h[i:i + ch]] + rel[r[i:i + ch]])[:, None, :] - ent[None]).norm(p=2, dim=-1) ** 2
            top, idx = s.sort(descending=True)
            top[:, :k], idx[:, :k]
    reference()
    torch.cuda.synchronize()
    base = statistics.median(timed(reference) for _ in range(3))
    row = dict(kernel="torch_broadcast_sort_baseline", n_ent=n_ent, dim=D, norm=2, queries=nq, chunk=ch, ms=round(base, 2),
               ms_per_4096_queries=round(base * 4096 / nq, 1))
    results.append(row)
    print(json.dumps(row), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(results, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
