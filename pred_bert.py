"""Applies the fine-tuned BERT pair classifier to a test file (reference pred_bert.py) on the HIP engine and writes the submission
lines: `deepAI_result_threshold=<t>.jsonl` under --output_dir, one line per test pair in file order, with the keys src_item_id,
tgt_item_id (the pair's text_id_a / text_id_b), src_item_emb = "[1 - p]", tgt_item_emb = "[p]" and threshold.

p is computed as the reference computes it: score = w . pool_out + b with (w, b) = BertAlignModel.get_sim_eval_weight(), then
p = 1 / (1 + exp(-score - b)) -- the bias enters twice.  Kept: the submitted numbers are the reference's.  The accuracy / precision /
recall / F1 line it prints takes pred = score > 0.  --model_name_or_path must be a local directory: nothing is ever downloaded (the
reference fetches its tokenizer by hub name).
"""
import argparse
import json
import os
import sys

os.environ.setdefault("HF_HUB_OFFLINE", "1")
os.environ.setdefault("TRANSFORMERS_OFFLINE", "1")

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def get_parser():
    from finetune_bert import add_length_flags
    p = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    a = p.add_argument
    a("--data_dir", required=True, type=str)
    a("--output_dir", required=True, type=str)
    a("--model_name_or_path", required=True, type=str, help="LOCAL directory with vocab.txt and config.json")
    a("--model_file", default=None, type=str, help="state_dict to apply (keys may carry a module. prefix); default "
      "<output_dir>/F1Model/pytorch_model.bin")
    a("--test_file", default="item-align-test.json", type=str)
    a("--batch_size", default=16, type=int)
    a("--threshold", default=0.4, type=float, help="written into every line; the reference's file name and value say 0.4")
    add_length_flags(a)
    return p


def metrics(preds, labels):
    """the reference's closing line (its 0.0001 in every denominator included)"""
    tp = sum(1 for p, t in zip(preds, labels) if p == t and t == 1)
    tn = sum(1 for p, t in zip(preds, labels) if p == t and t == 0)
    fn = sum(1 for p, t in zip(preds, labels) if p != t and t == 1)
    fp = sum(1 for p, t in zip(preds, labels) if p != t and t == 0)
    acc = (tp + tn) / (tp + tn + fp + fn + 0.0001)
    pre = tp / (tp + fp + 0.0001)
    recall = tp / (tp + fn + 0.0001)
    f1 = (2 * pre * recall) / (recall + pre + 0.0001)
    print("acc:", acc, "pre:", pre, "recall:", recall, "F1:", f1)
    return acc, pre, recall, f1


def main(argv=None):
    args = get_parser().parse_args(argv)
    from item_alignment_amd.cli_common import check_model_dir, load_config, load_vocab_tokenizer
    check_model_dir(args.model_name_or_path)
    model_file = args.model_file or os.path.join(args.output_dir, "F1Model", "pytorch_model.bin")
    if not os.path.isfile(model_file):
        raise SystemExit(f"--model_file {model_file!r} does not exist")
    import torch
    import item_alignment_amd.models as M
    from finetune_bert import check_lengths, forward, lengths_of, load_pairs, load_state_file
    from item_alignment_amd.data import bert_align as D

    config = load_config(os.path.join(args.model_name_or_path, "config.json"))
    check_lengths(args, config)
    if not torch.cuda.is_available():
        raise SystemExit("pred_bert.py runs on the MI355X HIP engine only (no CPU path); no GPU is visible")
    device = torch.device("cuda", int(os.environ.get("LOCAL_RANK", "0")))
    torch.cuda.set_device(device)

    tokenizer = load_vocab_tokenizer(os.path.join(args.model_name_or_path, "vocab.txt"))
    ids = D.read_data(args.data_dir, args.test_file, ["text_id_a", "text_id_b"])
    loader = load_pairs(args.data_dir, args.test_file, args.batch_size, tokenizer, "test", lengths_of(args))
    model = M.BertAlignModel(config)
    D.LOGGER.info(f"Loaded {load_state_file(model, model_file)} tensors from {model_file}")
    model.to(device).eval()

    pooled = []
    with torch.no_grad():
        for batch in loader:
            pooled.append(forward(model, batch, device, with_labels=False)[0][0].float().cpu())
    pooled = torch.cat(pooled, dim=0)
    assert len(ids) == pooled.shape[0]
    weight, bias = model.get_sim_eval_weight()
    os.makedirs(args.output_dir, exist_ok=True)
    out_file = os.path.join(args.output_dir, f"deepAI_result_threshold={args.threshold}.jsonl")
    preds, labels = [], []
    with open(out_file, "w", encoding="utf-8") as f:
        for (id_a, id_b, label), emb in zip(ids, pooled):
            score, prob = D.pred_probability(weight, bias, emb)
            f.write(json.dumps({"src_item_id": id_a, "tgt_item_id": id_b, "src_item_emb": str([1 - prob]), "tgt_item_emb": str([prob]),
                                "threshold": args.threshold}, ensure_ascii=False) + "\n")
            preds.append(1.0 if score > 0.0 else 0.0)
            labels.append(label)
    D.LOGGER.info(f"{len(ids)} lines written to {out_file}")
    metrics(preds, labels)
    return 0


if __name__ == "__main__":
    sys.exit(main())
