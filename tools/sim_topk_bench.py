"""Time of same-item retrieval (mine_items.py, ia_sim_topk) on one GPU at the shapes of tools/pkgm_infer_bench.py: a 258 211 x 768
catalogue of normalised rows, k = 10; 4 096 queries in one call, and the all-pairs run (every row queries the catalogue, itself
skipped, 4 096 queries a call).  In the same process, on the same bf16 rows:
  (a) chunked torch.matmul of the bf16 rows + torch.topk -- the [chunk, n] score matrix in HBM, the formulation the kernel replaces;
  (b) kg_topk (L2, fp32 rows, vector ALU) at the 4 096-query shape, for scale only.
The arms alternate (one order, then the reverse) after a warm-up, four rounds; the medians of the device-event times are reported, with
the achieved TFLOP/s (2 B n D) and the bytes per second of candidate stream the scan asks of the memory system (every query tile walks
the whole catalogue once: query_tiles x n x pitch x 2 bytes; how much of it HBM serves is what the L2 / Infinity Cache sharing decides).

    python tools/sim_topk_bench.py [--out profiles/sim_topk_bench.json] [--n 258211] [--dim 768] [--batch 4096] [--rounds 4]
    rocprofv3 --kernel-trace --stats -d <dir> -- python tools/sim_topk_bench.py --profile     (the kernel alone, in a run of its own)
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
    ap.add_argument("--n", type=int, default=258211)
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--top_k", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--no_all_pairs", action="store_true")
    ap.add_argument("--profile", action="store_true", help="three ia_sim_topk calls at the batch shape and nothing else")
    args = ap.parse_args()
    import torch
    from item_alignment_amd import retrieval as R
    from item_alignment_amd.models import kg_pretrain as K
    if not torch.cuda.is_available():
        raise SystemExit("sim_topk_bench.py measures on the GPU")
    dev = torch.device("cuda:0")
    n, D, B, k = args.n, args.dim, args.batch, args.top_k
    g = torch.Generator(device=dev).manual_seed(D)
    x = torch.randn(n, D, device=dev, generator=g)
    cand = R.prepare_rows(x, True)
    pitch = cand.shape[1]
    qsel = torch.randint(0, n, (B,), device=dev, generator=g)
    q = cand[qsel].contiguous()
    ws = torch.empty(R._lib.load().ia_sim_topk_workspace_bytes(B, D, n, k, 0), device=dev, dtype=torch.uint8)
    q_tile = 256 if k <= 32 else 128

    def sim(qq=q, skip=None):
        return R.sim_topk(qq, cand, D, k, skip=skip, workspace=ws)

    if args.profile:
        for _ in range(3):
            sim()
        torch.cuda.synchronize()
        return

    def torch_topk(qq=q):
        return (qq @ cand.T).topk(k, dim=1)

    ent = x * 0.05                                             # (b): fp32 rows, q = ent[a] + rel[0], rel = 0
    rel = torch.zeros(1, D, device=dev)
    zeros = torch.zeros(B, dtype=torch.int64, device=dev)
    ws_kg = torch.empty(R._lib.load().ia_kgpt_topk_workspace_bytes(B, D, n, k, 0), device=dev, dtype=torch.uint8)

    def kg():
        return K.kg_topk(ent, rel, qsel, zeros, 2, K.TOPK_TAILS, k, workspace=ws_kg)

    def sim_all():
        for lo in range(0, n, B):
            hi = min(n, lo + B)
            sim(cand[lo:hi], torch.arange(lo, hi, device=dev))

    def torch_all():
        for lo in range(0, n, B):
            s = cand[lo:lo + B] @ cand.T
            s[torch.arange(s.shape[0], device=dev), torch.arange(lo, lo + s.shape[0], device=dev)] = float("-inf")
            s.topk(k, dim=1)

    def timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b)

    def race(arms, warm):
        for fn in arms.values():
            for _ in range(warm):
                fn()
        torch.cuda.synchronize()
        ms = {name: [] for name in arms}
        for rnd in range(args.rounds):
            for name in (list(arms) if rnd % 2 == 0 else list(arms)[::-1]):
                ms[name].append(timed(arms[name]))
        return ms

    # the kernel's answer against fp32 products of the same bf16 rows (the bar of tests/simtopk_reference.py, once for each side)
    idx, score = sim(q[:8])
    exact = q[:8].float() @ cand.float().T
    bar = (pitch + 2) * 2.0 ** -23 * (q[:8].float().abs() @ cand.float().abs().T)
    assert ((score - exact.gather(1, idx)).abs() <= 2 * bar.gather(1, idx)).all()
    kth = exact.topk(k, dim=1).values[:, -1:]
    assert (exact.gather(1, idx) >= kth - 2 * bar.max()).all()

    results = []

    def report(name, queries, ms, base=None):
        med = statistics.median(ms)
        flop = 2.0 * queries * n * D
        row = dict(arm=name, n=n, dim=D, queries=queries, top_k=k, rounds=args.rounds, ms=round(med, 2),
                   spread_ms=[round(min(ms), 2), round(max(ms), 2)], tflops=round(flop / (med * 1e-3) / 1e12, 1))
        if name.startswith("sim_topk"):
            stream = -(-min(queries, B) // q_tile) * -(-queries // B) * float(n) * pitch * 2
            row.update(candidate_stream_bytes=stream, candidate_stream_TBps=round(stream / (med * 1e-3) / 1e12, 2),
                       catalogue_bytes=n * pitch * 2, workspace_bytes=ws.numel(), matrix_bytes_avoided=4 * queries * n)
        if base is not None:
            row["ratio_to_torch_matmul_topk"] = round(med / statistics.median(base), 3)
        results.append(row)
        print(json.dumps(row), flush=True)

    ms = race({"sim": sim, "torch": torch_topk, "kg": kg}, 2)
    report("sim_topk_4096", B, ms["sim"], ms["torch"])
    report("torch_matmul_topk_4096", B, ms["torch"])
    report("kg_topk_l2_4096_for_scale", B, ms["kg"])
    if not args.no_all_pairs:
        ms = race({"sim": sim_all, "torch": torch_all}, 1)
        report("sim_topk_all_pairs", n, ms["sim"], ms["torch"])
        report("torch_matmul_topk_all_pairs", n, ms["torch"])
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(results, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
