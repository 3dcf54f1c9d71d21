"""Throughput of link-prediction ranking (pkgm_pretrain.py --do_test, ia_kgpt_lp_rank) on one GPU at the CCKS shape: 258 211 entities,
1 379 relations, D in {768, 1024}, B queries per call, both sides of every fact, L2 and L1.  One JSON line per (D, norm): facts/s
(both sides), element pairs/s (2 n_ent D per fact) and the fraction of the fp32 VALU ceiling (one subtract and one FMA per pair:
157.3 TFLOPS / 4 = 3.93e13 pairs/s), unfiltered; then L2 with the filter correction, for 16-member groups and for one group of
100 000 members that every query falls in (of_unfiltered = unfiltered time / filtered time).  Then the baseline: the reference's own broadcast arithmetic (inference_scoring_function's
-(h + r - c).norm(dim=-1)**2 and get_rank) in plain torch on the same GPU, in query chunks that fit.

    python tools/pkgm_linkpred_bench.py [--batch 4096] [--dims 768 1024] [--reps 3] [--baseline_queries 64]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
VALU_PAIRS_PER_S = 157.3e12 / 4


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--dims", type=int, nargs="+", default=[768, 1024])
    ap.add_argument("--norms", type=int, nargs="+", default=[2, 1])
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--baseline_queries", type=int, default=64)
    ap.add_argument("--baseline_chunk", type=int, default=4)
    ap.add_argument("--heavy_group", type=int, default=100000)
    args = ap.parse_args()
    import numpy as np
    import torch
    from item_alignment_amd.models import kg_pretrain as K
    rng = np.random.default_rng(0)
    n_ent, n_rel, B = 258211, 1379, args.batch
    dev = torch.device("cuda:0")
    for D in args.dims:
        unfiltered_ms = None
        g = torch.Generator(device=dev).manual_seed(D)
        ent = torch.randn(n_ent, D, device=dev, generator=g) * 0.05
        rel = torch.randn(n_rel, D, device=dev, generator=g) * 0.05
        h, t = (torch.randint(0, n_ent, (B,), device=dev, generator=g) for _ in range(2))
        r = torch.randint(0, n_rel, (B,), device=dev, generator=g)
        ws = torch.empty(K._lib.load().ia_kgpt_lp_workspace_bytes(B, D), device=dev, dtype=torch.uint8)
        for norm in args.norms:
            def run():
                for side in (K.LP_TAIL, K.LP_HEAD):
                    K.lp_rank(ent, rel, h, t, r, norm, side, workspace=ws)
            run()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(args.reps):
                run()
            torch.cuda.synchronize()
            dt = (time.perf_counter() - t0) / args.reps
            pairs = 2.0 * B * n_ent * D
            if norm == 2:
                unfiltered_ms = dt * 1e3
            print(json.dumps(dict(kernel="ia_kgpt_lp_rank", filter=None, n_ent=n_ent, n_rel=n_rel, dim=D, norm=norm, batch=B, ms_per_batch=round(dt * 1e3, 2),
                                  facts_per_s=round(B / dt), pairs_per_s=float(f"{pairs / dt:.4g}"),
                                  of_valu_ceiling=round(pairs / dt / VALU_PAIRS_PER_S, 3),
                                  ceiling_facts_per_s=round(VALU_PAIRS_PER_S / (2 * n_ent * D)))), flush=True)
        # the filter correction (listed mode over each query's group), L2: a typical group of 16 members per query, and one shared
        # group of 100 000 members (a popular category) that every query falls in
        typ_ids = np.sort(np.concatenate([t.cpu().numpy()[:, None], rng.integers(0, n_ent, (B, 15))], 1), 1).reshape(-1)
        typical = K.FilterGroups(np.arange(B, dtype=np.int64), np.arange(0, 16 * B + 1, 16, dtype=np.int64), typ_ids, 1)
        heavy = K.FilterGroups(np.zeros(1, np.int64), np.array([0, args.heavy_group], np.int64),
                               np.sort(rng.permutation(n_ent)[:args.heavy_group]).astype(np.int64), 1)
        for gname, groups, qg in (("typical_16", typical, np.arange(B)), (f"shared_{args.heavy_group}", heavy, np.zeros(B, np.int64))):
            dg = K._DeviceGroups(groups, dev)
            qg = torch.from_numpy(qg).to(dev)

            def run_f():
                for side in (K.LP_TAIL, K.LP_HEAD):
                    K.lp_rank(ent, rel, h, t, r, 2, side, dg, qg, workspace=ws)
            run_f()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            run_f()
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            print(json.dumps(dict(kernel="ia_kgpt_lp_rank", filter=gname, n_ent=n_ent, dim=D, norm=2, batch=B, ms_per_batch=round(dt * 1e3, 2),
                                  facts_per_s=round(B / dt), of_unfiltered=round(unfiltered_ms / (dt * 1e3), 3) if unfiltered_ms else None)), flush=True)
        # baseline: the reference's broadcast in plain torch ([chunk, n_ent, D] fp32 per call), L2, both sides
        nq, ch = args.baseline_queries, args.baseline_chunk

        def ref_ranks():
            for i in range(0, nq, ch):
                hh, tt, rr = h[i:i + ch], t[i:i + ch], r[i:i + ch]
                s = -((ent[hh] + rel[rr])[:, None, :] - ent[None]).norm(p=2, dim=-1) ** 2
                (s >= s.gather(1, tt[:, None])).sum(1)
                s = -((ent[None] + rel[rr][:, None, :]) - ent[tt][:, None, :]).norm(p=2, dim=-1) ** 2
                (s >= s.gather(1, hh[:, None])).sum(1)
        ref_ranks()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ref_ranks()
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        print(json.dumps(dict(kernel="torch_broadcast_baseline", n_ent=n_ent, dim=D, norm=2, queries=nq, chunk=ch,
                              facts_per_s=round(nq / dt, 1), pairs_per_s=float(f"{2.0 * nq * n_ent * D / dt:.4g}"))), flush=True)
        del ent, rel, ws
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
