"""Same-item mining: for every item of a catalogue of embeddings its --top_k most similar items on the bf16 MFMA similarity top-k
kernels: exact (--index flat, the default: ia_sim_topk through item_alignment_amd.retrieval.ItemIndex) or through an inverted-file
index that scans only the --nprobe lists nearest to a query (--index ivf: ia_sim_topk_groups through retrieval.IVFItemIndex).

    --embeddings        feature_matrix.pt (with --ids_file entity2id.txt; pred_text.py), image_embedding.json (image_embedding.py) or a
                        two-tower deepAI_result_*.jsonl (--do_pred: src_item_emb / tgt_item_emb, the first occurrence of an id wins)
    --query_embeddings  the same formats; default: the catalogue queries itself and no item lists itself

Output, one JSON line per query in query order: {"item_id": ..., "neighbours": [ids ...], "scores": [...]}, best first in the order
(score descending, catalogue row ascending); entries below --min_score and unused slots are left out.  --pairs_file (an item_*_pair.jsonl
with src_item_id, tgt_item_id, item_label) prints `recall@K=... mrr@K=... positives=... skipped=...` over its label-1 pairs.
--index ivf: --nlist (default round(4 sqrt(N))), --nprobe, --train_size, --kmeans_iters and --seed shape the index; --index_file loads
it if the file exists, else trains and saves it; --recall_check Q searches the first Q queries of a seeded permutation exactly too and
prints `ivf_recall@K=... over Q queries (nprobe=..., nlist=...)`, the share of the exact lists' entries the ivf lists contain: how to
pick --nprobe.  INTEGRATION.md section 10 describes the flow, what --nprobe trades and what bf16 storage does to a score (--rescore).
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


# the flags of --index ivf alone; unset (None) they take the defaults of IVFItemIndex
IVF_FLAGS = (("nlist", int, "number of lists (default round(4 sqrt(N)))"), ("nprobe", int, "lists scanned per query (default 16)"),
             ("train_size", int, "rows of the k-means sample (default min(N, 256 nlist))"), ("kmeans_iters", int, "default 10"),
             ("seed", int, "of the sample and the start (default 0)"), ("index_file", str, "load the index if it exists, else train and save"),
             ("recall_check", int, "Q: compare Q queries with the exact search and print ivf_recall@K"))


def get_parser():
    parser = argparse.ArgumentParser()
    parser.add_argument("--embeddings", required=True, type=str, help="the catalogue: .pt, .json or .jsonl")
    parser.add_argument("--ids_file", default=None, type=str, help="with a .pt catalogue: one id per line (first tab-separated column)")
    parser.add_argument("--query_embeddings", default=None, type=str, help="default: the catalogue itself, self excluded")
    parser.add_argument("--query_ids_file", default=None, type=str)
    parser.add_argument("--metric", default="cosine", type=str, help="cosine or ip")
    parser.add_argument("--top_k", default=10, type=int)
    parser.add_argument("--batch_size", default=4096, type=int, help="queries per kernel call")
    parser.add_argument("--rescore", action="store_true", help="report fp32 scores of the returned neighbours")
    parser.add_argument("--min_score", default=None, type=float, help="drop neighbours scoring below it")
    parser.add_argument("--output_file", required=True, type=str)
    parser.add_argument("--pairs_file", default=None, type=str, help="labelled pairs for recall@K")
    parser.add_argument("--index", default="flat", type=str, help="flat (exact) or ivf (inverted file, approximate)")
    for flag, kind, text in IVF_FLAGS:
        parser.add_argument(f"--{flag}", default=None, type=kind, help=f"--index ivf: {text}")
    return parser


def check_args(args):
    if args.metric not in ("cosine", "ip"):
        raise SystemExit(f"--metric {args.metric}: use cosine or ip")
    if not 1 <= args.top_k <= 64:
        raise SystemExit(f"--top_k {args.top_k}: the top-k kernel keeps between 1 and 64 candidates per query")
    if args.batch_size <= 0:
        raise SystemExit(f"--batch_size {args.batch_size}: needs a positive batch size")
    if args.index not in ("flat", "ivf"):
        raise SystemExit(f"--index {args.index}: use flat or ivf")
    if args.index == "flat":
        for flag, _, _ in IVF_FLAGS:
            if getattr(args, flag) is not None:
                raise SystemExit(f"--{flag} shapes the inverted-file index: it needs --index ivf")
    if args.nprobe is not None and args.nprobe < 1:
        raise SystemExit(f"--nprobe {args.nprobe}: a query scans at least one list")
    if args.nlist is not None and args.nlist < 1:
        raise SystemExit(f"--nlist {args.nlist}: needs between 1 and N lists")
    for flag in ("train_size", "kmeans_iters", "recall_check"):
        if getattr(args, flag) is not None and getattr(args, flag) < (0 if flag == "kmeans_iters" else 1):
            raise SystemExit(f"--{flag} {getattr(args, flag)}: needs a positive number")
    if args.query_ids_file and not args.query_embeddings:
        raise SystemExit("--query_ids_file names the rows of --query_embeddings: it needs that flag")
    for flag in ("embeddings", "ids_file", "query_embeddings", "query_ids_file", "pairs_file"):
        path = getattr(args, flag)
        if path is not None and not os.path.isfile(path):
            raise SystemExit(f"--{flag}: {path} does not exist")
    for flag, path, ids in (("embeddings", args.embeddings, args.ids_file), ("query_embeddings", args.query_embeddings, args.query_ids_file)):
        if path is not None and not path.endswith((".pt", ".json", ".jsonl")):
            raise SystemExit(f"--{flag} {path}: unknown embedding format (use .pt, .json or .jsonl)")
        if ids is not None and not path.endswith(".pt"):
            raise SystemExit(f"--{flag} {path}: an ids file goes with a .pt matrix only (the other formats carry their ids)")


def read_pairs(path):
    pairs = []
    with open(path, "r", encoding="utf-8") as f:
        for no, line in enumerate(f, 1):
            if not line.strip():
                continue
            try:
                rec = json.loads(line)
                pairs.append((str(rec["src_item_id"]), str(rec["tgt_item_id"]), int(rec["item_label"])))
            except (ValueError, KeyError, TypeError):
                raise SystemExit(f"--pairs_file {path} line {no}: expected src_item_id, tgt_item_id and item_label")
    return pairs


def build_ivf(R, args, x, ids):
    """the index of --index_file if that file exists; else a trained one, saved there if the flag is given"""
    kw = {flag: getattr(args, flag) for flag in ("nprobe", "train_size", "kmeans_iters", "seed") if getattr(args, flag) is not None}
    try:
        if args.index_file and os.path.isfile(args.index_file):
            for flag in ("train_size", "kmeans_iters", "seed"):
                kw.pop(flag, None)                            # they shaped the training the file already holds
            index = R.IVFItemIndex.load(args.index_file, x, ids, metric=args.metric, keep_fp32=args.rescore, **kw)
            if args.nlist is not None and args.nlist != index.nlist:
                raise SystemExit(f"--nlist {args.nlist}: --index_file {args.index_file} holds {index.nlist} lists")
            return index
        index = R.IVFItemIndex(x, ids, args.metric, nlist=args.nlist, keep_fp32=args.rescore, **kw)
    except ValueError as e:
        raise SystemExit(f"--index ivf: {e}")
    if args.index_file:
        index.save(args.index_file)
    return index


def main(argv=None):
    args = get_parser().parse_args(argv)
    check_args(args)
    import torch
    from item_alignment_amd import retrieval as R

    def load(flag, path, ids_file):
        try:
            return R.load_embeddings(path, ids_file)
        except ValueError as e:
            raise SystemExit(f"--{flag}: {e}")

    ids, x, differing = load("embeddings", args.embeddings, args.ids_file)
    q_ids, qx = ids, None
    if args.query_embeddings:
        q_ids, qx, q_differing = load("query_embeddings", args.query_embeddings, args.query_ids_file)
        differing += q_differing
        if qx.shape[1] != x.shape[1]:
            raise SystemExit(f"--query_embeddings {args.query_embeddings}: rows of {qx.shape[1]} numbers, the catalogue's have {x.shape[1]}")
    if args.nlist is not None and args.nlist > x.shape[0]:
        raise SystemExit(f"--nlist {args.nlist}: needs between 1 and N = {x.shape[0]} lists")
    pairs = read_pairs(args.pairs_file) if args.pairs_file else None
    if not torch.cuda.is_available():
        raise SystemExit("mine_items.py runs on the GPU (HIP kernels, no CPU path)")
    if differing:
        print(f"{differing} later occurrence(s) of an item id carry another embedding than the first; the first is used")
    if args.index == "ivf":
        index = build_ivf(R, args, x, ids)
        print(index.summary())
        nprobe = min(index.nprobe, index.nlist)
        idx, score = index.search(qx, k=args.top_k, batch_size=args.batch_size, rescore=args.rescore)
        if args.recall_check:
            g = torch.Generator().manual_seed(index.seed)
            nq = x.shape[0] if qx is None else qx.shape[0]
            sample = torch.randperm(nq, generator=g)[:args.recall_check]
            flat = R.ItemIndex(x, ids, args.metric, keep_fp32=False)
            if qx is None:                                    # the catalogue queries itself: row sample[i] is kept from query i
                exact = R.sim_topk(flat.rows[sample.to(flat.device)], flat.rows, x.shape[1], args.top_k, skip=sample)[0].cpu()
            else:
                exact = flat.search(qx[sample], k=args.top_k, batch_size=args.batch_size)[0]
            found = sum(len(set(e) & set(a)) for e, a in zip((r[r >= 0].tolist() for r in exact), idx[sample].tolist()))
            print(f"ivf_recall@{args.top_k}={found / max(int((exact >= 0).sum()), 1):.4f} over {sample.numel()} queries "
                  f"(nprobe={nprobe}, nlist={index.nlist})")
    else:
        index = R.ItemIndex(x, ids, args.metric, keep_fp32=args.rescore)
        idx, score = index.search(qx, k=args.top_k, batch_size=args.batch_size, rescore=args.rescore)
    lo = float("-inf") if args.min_score is None else args.min_score
    with open(args.output_file, "w", encoding="utf-8") as f:
        for item, row, sc in zip(q_ids, idx.tolist(), score.tolist()):
            keep = [(ids[c], s) for c, s in zip(row, sc) if c >= 0 and s >= lo]
            f.write(json.dumps({"item_id": item, "neighbours": [c for c, _ in keep], "scores": [s for _, s in keep]}, ensure_ascii=False) + "\n")
    if pairs is not None:
        recall, mrr, used, skipped = R.recall_at_k(idx, ids, pairs, None if qx is None else q_ids)
        print(f"recall@{args.top_k}={recall:.4f} mrr@{args.top_k}={mrr:.4f} positives={used} skipped={skipped}")


if __name__ == "__main__":
    main()
