"""Knowledge-graph completion with a trained PKGM / TransE checkpoint (torchkge inference.py EntityInference / RelationInference; the
reference has no script for it) on the streaming top-k kernel (ia_kgpt_topk).

    --missing tails:      query lines `head \\t rel`,  the --top_k best tails
    --missing heads:      query lines `tail \\t rel`,  the --top_k best heads
    --missing relations:  query lines `head \\t tail`, the --top_k best relations

Output, one line per (query, rank): `query_index \\t a \\t b \\t rank \\t id \\t name \\t score`, best first in the order (score
descending, id ascending); score is written with %.9g.  --filter_known leaves out the completions known from train2id.txt (and
valid2id.txt with --do_eval, test2id.txt with --do_test); a query with fewer than --top_k candidates left gets fewer lines.
INTEGRATION.md "PKGM knowledge-graph pretraining" lists the deviations from torchkge.
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def get_parser():
    parser = argparse.ArgumentParser()
    parser.add_argument("--data_dir", required=True, type=str, help="directory with entity2id.txt, relation2id.txt, train2id.txt")
    parser.add_argument("--model_path", required=True, type=str, help="a state dict written by pkgm_pretrain.py")
    parser.add_argument("--query_file", required=True, type=str, help="two tab-separated integer ids per line")
    parser.add_argument("--output_file", required=True, type=str)
    parser.add_argument("--missing", default="tails", type=str, help="tails, heads or relations")
    parser.add_argument("--top_k", default=10, type=int)
    parser.add_argument("--eval_batch_size", default=2048, type=int, help="queries per kernel call")
    parser.add_argument("--norm", default="L2", type=str, help="vector norm: L1 or L2")
    parser.add_argument("--filter_known", action="store_true", help="never return a completion that is a known fact")
    parser.add_argument("--do_eval", action="store_true", help="with --filter_known: valid2id.txt joins the known facts")
    parser.add_argument("--do_test", action="store_true", help="with --filter_known: test2id.txt joins the known facts")
    return parser


def _names(path):
    """id -> name of an id file (`name \\t id`)."""
    out = {}
    with open(path, "r", encoding="utf-8") as f:
        for line in f:
            if line.strip():
                name, i = line.rstrip("\n").split("\t")[:2]
                out[int(i)] = name
    return out


def check_args(args):
    if args.missing not in ("tails", "heads", "relations"):
        raise SystemExit(f"--missing {args.missing}: use tails, heads or relations")
    if not 1 <= args.top_k <= 64:
        raise SystemExit(f"--top_k {args.top_k}: the top-k kernel keeps between 1 and 64 candidates per query")
    if args.eval_batch_size <= 0:
        raise SystemExit(f"--eval_batch_size {args.eval_batch_size}: needs a positive batch size")
    if args.norm not in ("L1", "L2"):
        raise SystemExit(f"--norm {args.norm}: only L1 and L2 are supported (the torus dissimilarities are not built)")
    if (args.do_eval or args.do_test) and not args.filter_known:
        raise SystemExit("--do_eval / --do_test widen the filter: they need --filter_known")
    files = [("--data_dir", os.path.join(args.data_dir, f)) for f in ("entity2id.txt", "relation2id.txt", "train2id.txt")]
    files += [("--model_path", args.model_path), ("--query_file", args.query_file)]
    files += [(flag, os.path.join(args.data_dir, f)) for flag, on, f in (("--do_eval", args.do_eval, "valid2id.txt"),
                                                                         ("--do_test", args.do_test, "test2id.txt")) if on]
    for flag, path in files:
        if not os.path.isfile(path):
            raise SystemExit(f"{flag}: {path} does not exist")


def read_queries(path, missing, n_ent, n_rel):
    """The two id columns of the query file; an id outside its table is refused with its line number."""
    bounds = ((("head", n_ent), ("tail", n_ent)) if missing == "relations" else
              (("head" if missing == "tails" else "tail", n_ent), ("rel", n_rel)))
    a, b = [], []
    with open(path, "r", encoding="utf-8") as f:
        for no, line in enumerate(f, 1):
            if not line.strip():
                continue
            cols = line.rstrip("\n").split("\t")
            try:
                ids = [int(c) for c in cols]
            except ValueError:
                ids = []
            if len(ids) != 2:
                raise SystemExit(f"--query_file {path} line {no}: expected two tab-separated integer ids, got {line.rstrip()!r}")
            for v, (name, n) in zip(ids, bounds):
                if not 0 <= v < n:
                    raise SystemExit(f"--query_file {path} line {no}: {name} id {v} lies outside [0, {n})")
            a.append(ids[0])
            b.append(ids[1])
    return a, b


def main(argv=None):
    args = get_parser().parse_args(argv)
    check_args(args)
    import torch
    from item_alignment_amd.models import kg_pretrain as K

    ent_names, rel_names = (_names(os.path.join(args.data_dir, f)) for f in ("entity2id.txt", "relation2id.txt"))
    n_ent, n_rel = max(ent_names, default=-1) + 1, max(rel_names, default=-1) + 1
    sd = torch.load(args.model_path, map_location="cpu")
    for key, n in (("ent_emb.weight", n_ent), ("rel_emb.weight", n_rel)):
        if key not in sd or sd[key].dim() != 2:
            raise SystemExit(f"--model_path {args.model_path}: no 2-D table {key} (a state dict of pkgm_pretrain.py is expected)")
        if sd[key].shape[0] != n:
            raise SystemExit(f"--model_path {args.model_path}: {key} has {sd[key].shape[0]} rows, the id files of --data_dir have {n}")
    dim = sd["ent_emb.weight"].shape[1]
    if sd["rel_emb.weight"].shape[1] != dim or dim % 4:
        raise SystemExit(f"--model_path {args.model_path}: table widths {dim} / {sd['rel_emb.weight'].shape[1]} (one width, a multiple of "
                         "4, is expected)")
    a, b = read_queries(args.query_file, args.missing, n_ent, n_rel)
    groups = None
    if args.filter_known:
        try:
            train, valid, test, filters = K.load_ccks_splits(args.data_dir, args.do_eval, args.do_test)
        except ValueError as e:
            raise SystemExit(f"--filter_known: {e}")
        groups = (filters.tails if args.missing == "tails" else filters.heads if args.missing == "heads" else
                  K.relation_filter_groups([train, valid, test]))
    if not torch.cuda.is_available():
        raise SystemExit("pkgm_infer.py runs on the GPU (HIP kernels, no CPU path)")
    model = K.TransEPretrainModel(dim, n_ent, n_rel, dissimilarity_type=args.norm)        # proj_mat.weight is not used for scoring
    model.load_state_dict({k: sd[k].float() for k in ("ent_emb.weight", "rel_emb.weight")})
    model = model.cuda()
    a, b = torch.tensor(a, dtype=torch.int64), torch.tensor(b, dtype=torch.int64)
    if args.missing == "relations":
        inf = K.RelationInference(model, a, b, top_k=args.top_k, dictionary=groups)
    else:
        inf = K.EntityInference(model, a, b, top_k=args.top_k, missing=args.missing, dictionary=groups)
    inf.evaluate(args.eval_batch_size, verbose=False)
    names = rel_names if args.missing == "relations" else ent_names
    pred, score = inf.predictions.tolist(), inf.scores.tolist()
    with open(args.output_file, "w", encoding="utf-8") as f:
        for i, (qa, qb) in enumerate(zip(a.tolist(), b.tolist())):
            for rank, (c, s) in enumerate(zip(pred[i], score[i]), 1):
                if c >= 0:
                    f.write(f"{i}\t{qa}\t{qb}\t{rank}\t{c}\t{names.get(c, '')}\t{s:.9g}\n")


if __name__ == "__main__":
    main()
