"""Same-item mining: for every item of a catalogue of embeddings its --top_k most similar items, exact, on the bf16 MFMA similarity
top-k kernel (ia_sim_topk through item_alignment_amd.retrieval.ItemIndex).

    --embeddings        feature_matrix.pt (with --ids_file entity2id.txt; pred_text.py), image_embedding.json (image_embedding.py) or a
                        two-tower deepAI_result_*.jsonl (--do_pred: src_item_emb / tgt_item_emb, the first occurrence of an id wins)
    --query_embeddings  the same formats; default: the catalogue queries itself and no item lists itself

Output, one JSON line per query in query order: {"item_id": ..., "neighbours": [ids ...], "scores": [...]}, best first in the order
(score descending, catalogue row ascending); entries below --min_score and unused slots are left out.  --pairs_file (an item_*_pair.jsonl
with src_item_id, tgt_item_id, item_label) prints `recall@K=... mrr@K=... positives=... skipped=...` over its label-1 pairs.
INTEGRATION.md section 10 describes the flow and what bf16 storage does to a score (--rescore).
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


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
    return parser


def check_args(args):
    if args.metric not in ("cosine", "ip"):
        raise SystemExit(f"--metric {args.metric}: use cosine or ip")
    if not 1 <= args.top_k <= 64:
        raise SystemExit(f"--top_k {args.top_k}: the top-k kernel keeps between 1 and 64 candidates per query")
    if args.batch_size <= 0:
        raise SystemExit(f"--batch_size {args.batch_size}: needs a positive batch size")
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
    pairs = read_pairs(args.pairs_file) if args.pairs_file else None
    if not torch.cuda.is_available():
        raise SystemExit("mine_items.py runs on the GPU (HIP kernels, no CPU path)")
    if differing:
        print(f"{differing} later occurrence(s) of an item id carry another embedding than the first; the first is used")
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
