"""Time and recall of same-item mining through the inverted-file index (retrieval.IVFItemIndex, ia_sim_topk_groups) against the exact
index (retrieval.ItemIndex, ia_sim_topk) on one GPU, in one process, on the same rows.

Rows: a seeded mixture -- `centres` unit directions, every row one of them plus Gaussian noise of norm about `noise` -- because an
inverted file lives on neighbourhood structure; on uniform random rows every list is as good as any other and a recall says nothing.
The generator's parameters are written into the JSON.  Shapes: 258 211 x 768 (the shape of tools/sim_topk_bench.py) and 2 000 000 x 256.

Per shape: the build, and the share of it that is k-means (a build without iterations timed beside it), then all-pairs mining (every
row queries the catalogue, itself skipped, k = 10) by the exact index and by the inverted file at nprobe in {1, 4, 16, 64}: wall time
around search(), which ends in the copies of the lists to the host, after a warm-up of every arm, the arms in one order and then in the
reverse; recall@10 of each nprobe = the share of the exact lists' entries of a fixed 16 384-query sample that its lists contain.  An
inverted-file call takes as many queries as give `--max_rows` (query, probe) rows, so that a list meets a tile's worth of queries.

    python tools/ivf_bench.py [--out profiles/ivf_bench.json] [--shapes 258211x768,2000000x256] [--rounds 2]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

NPROBES = (1, 4, 16, 64)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--shapes", default="258211x768,2000000x256")
    ap.add_argument("--top_k", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--rows_per_centre", type=int, default=100)
    ap.add_argument("--noise", type=float, default=0.7)
    ap.add_argument("--sample", type=int, default=16384)
    ap.add_argument("--max_rows", type=int, default=1 << 21, help="(query, probe) rows of one inverted-file call")
    ap.add_argument("--seed", type=int, default=0)
    args = ap.parse_args()
    import torch
    from item_alignment_amd import retrieval as R
    if not torch.cuda.is_available():
        raise SystemExit("ivf_bench.py measures on the GPU")
    dev = torch.device("cuda:0")
    k = args.top_k
    results = []

    def wall(fn):
        torch.cuda.synchronize()
        t = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return out, (time.perf_counter() - t) * 1e3

    for shape in args.shapes.split(","):
        n, D = (int(v) for v in shape.split("x"))
        centres = max(1, n // args.rows_per_centre)
        g = torch.Generator(device=dev).manual_seed(args.seed + D)
        c = torch.nn.functional.normalize(torch.randn(centres, D, device=dev, generator=g), dim=1)
        x = c[torch.randint(0, centres, (n,), device=dev, generator=g)]
        x += torch.randn(n, D, device=dev, generator=g) * (args.noise / D ** 0.5)
        del c
        data = dict(n=n, dim=D, generator="unit centres + Gaussian noise", centres=centres, noise_norm=args.noise, seed=args.seed + D)

        flat, flat_ms = wall(lambda: R.ItemIndex(x, keep_fp32=False))
        R.IVFItemIndex(x, keep_fp32=False, seed=args.seed, kmeans_iters=1)                    # warm-up of the build's kernels
        _, bare_ms = wall(lambda: R.IVFItemIndex(x, keep_fp32=False, seed=args.seed, kmeans_iters=0))
        index, build_ms = wall(lambda: R.IVFItemIndex(x, keep_fp32=False, seed=args.seed))
        row = dict(data, arm="build", nlist=index.nlist, kmeans_iters=10, ivf_build_ms=round(build_ms, 1),
                   ivf_build_without_kmeans_ms=round(bare_ms, 1), kmeans_share=round(1 - bare_ms / build_ms, 3), flat_build_ms=round(flat_ms, 1),
                   lists=index.summary())
        results.append(row)
        print(json.dumps(row), flush=True)

        arms = {"exact": lambda: flat.search(k=k, batch_size=4096)}
        batch = {}
        for nprobe in NPROBES:
            if nprobe > index.nlist:
                continue
            batch[nprobe] = max(1, args.max_rows // nprobe)
            arms[f"ivf_nprobe{nprobe}"] = lambda p=nprobe: index.search(k=k, nprobe=p, batch_size=batch[p])
        found = {name: fn()[0] for name, fn in arms.items()}    # the warm-up of every arm; its lists give the recall
        sample = torch.randperm(n, generator=torch.Generator().manual_seed(args.seed))[:args.sample]
        want = found["exact"][sample]
        ms = {name: [] for name in arms}
        for rnd in range(args.rounds):
            for name in (list(arms) if rnd % 2 == 0 else list(arms)[::-1]):
                ms[name].append(wall(arms[name])[1])
        exact_ms = statistics.median(ms["exact"])
        for name in arms:
            got = found[name][sample]
            hit = ((want[:, :, None] == got[:, None, :]) & (want[:, :, None] >= 0)).any(2).sum().item()
            med = statistics.median(ms[name])
            row = dict(data, arm=name, top_k=k, nlist=index.nlist, queries=n, rounds=args.rounds, all_pairs_ms=round(med, 1),
                       spread_ms=[round(min(ms[name]), 1), round(max(ms[name]), 1)], ratio_to_exact=round(med / exact_ms, 3),
                       recall_at_k=round(hit / max(int((want >= 0).sum()), 1), 4), recall_queries=int(sample.numel()))
            if name != "exact":
                row.update(nprobe=int(name[len("ivf_nprobe"):]), queries_per_call=min(n, batch[int(name[len("ivf_nprobe"):])]))
            results.append(row)
            print(json.dumps(row), flush=True)
        del flat, index, x, found
        torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(results, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
