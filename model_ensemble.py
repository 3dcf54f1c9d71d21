#!/usr/bin/env python3
"""Fuses the prediction files of several models into the submission file: the reference's model_ensemble.py (flags :75-87, accumulation
:90-197, fusion and output :200-254).  Host only.

Every member is a directory under <data_dir>/output/ holding --input_file, the deepAI_result_threshold=*.jsonl a finetune / pred script
wrote, with its threshold and its validation F1.  Per pair (src_item_id-tgt_item_id) the members' `prob - threshold` are summed and
their votes counted with weight F1 under the keys '1' (prob >= threshold) and '0'; the first member's record of the pair is the base of
the fused record.  --ensemble_strategy threshold writes the sum as the score, f1 writes 1.0 where the '1' votes weigh at least as much
as the '0' votes and -1.0 elsewhere.  The fused records go to <data_dir>/output/ensemble/deepAI_result.jsonl with tgt_item_emb "[score]"
and threshold 0.0.

--split_by_valid_or_test: pairs with an item whose cate_name is one of `unseen_categories` are fused from `members_not_in_train`, all
the others from `members_in_train`.

The member lists come from --members_file (the reference keeps them as literals in its source), a JSON object:
    {"members": [[dir, threshold, f1], ...], "members_in_train": [...], "members_not_in_train": [...], "unseen_categories": [...]}
Only the lists the chosen mode reads have to be there.  The embedding string is parsed as data (json, ast.literal_eval), never evaluated.
"""
import argparse
import ast
import copy
import json
import os

STRATEGIES = ("threshold", "f1")


def build_parser():
    parser = argparse.ArgumentParser()
    a = parser.add_argument
    a("--data_dir", required=True, type=str, help="data directory: raw/item_info.jsonl and output/<member>/<input_file> are read")
    a("--ensemble_strategy", required=True, type=str, help="threshold: sum of (prob - threshold); f1: F1-weighted vote")
    a("--input_file", default="deepAI_result_threshold=0.4.jsonl", type=str, help="name of the prediction file in every member directory")
    a("--split_by_valid_or_test", action="store_true", help="use other members and thresholds for pairs of a category the training data lacks")
    # not in the reference
    a("--members_file", required=True, type=str, help="JSON file with the member lists (see the module docstring)")
    return parser


def first_score(text):
    """first number of an embedding string such as "[0.73]" or "[0.1,0.9]" """
    try:
        v = json.loads(text)
    except ValueError:
        v = ast.literal_eval(text)
    return v[0]


def accumulate(lines, args, id_dict, members, keep):
    """reference :94-126: one pass over every member's file; keep(src category, tgt category) selects the pairs"""
    from item_alignment_amd.utils import logger
    for model, threshold, f1 in members:
        ct = total = 0
        with open(os.path.join(args.data_dir, "output", model, args.input_file), "r", encoding="utf-8") as r:
            for line in r:
                if not line.strip():
                    continue
                d = json.loads(line.strip())
                src, tgt = d["src_item_id"], d["tgt_item_id"]
                if not keep(id_dict[src]["cate_name"], id_dict[tgt]["cate_name"]):
                    continue
                key = src + "-" + tgt
                prob = first_score(d["tgt_item_emb"])
                if key not in lines:
                    dd = copy.deepcopy(d)
                    dd["tgt_item_emb"] = prob - threshold
                    dd["0"] = 0.0
                    dd["1"] = 0.0
                    lines[key] = dd
                else:
                    lines[key]["tgt_item_emb"] += prob - threshold
                if prob >= threshold:
                    ct += 1
                    lines[key]["1"] += f1
                else:
                    lines[key]["0"] += f1
                total += 1
        logger.info(f"{model}-{threshold} p: {ct}, total: {total}")


def ensemble(args, id_dict, members):
    lines = {}
    if args.split_by_valid_or_test:
        unseen = set(members["unseen_categories"])
        accumulate(lines, args, id_dict, members["members_in_train"], lambda s, t: not (s in unseen or t in unseen))
        accumulate(lines, args, id_dict, members["members_not_in_train"], lambda s, t: s in unseen or t in unseen)
    else:
        accumulate(lines, args, id_dict, members["members"], lambda s, t: True)
    return lines


def main(argv=None):
    args = build_parser().parse_args(argv)
    if args.ensemble_strategy not in STRATEGIES:
        raise ValueError(f"unsupported ensemble strategy: {args.ensemble_strategy}")
    from item_alignment_amd.data.graph_files import read_item_info
    from item_alignment_amd.utils import logger
    with open(args.members_file, "r", encoding="utf-8") as f:
        members = json.load(f)
    need = ("members_in_train", "members_not_in_train", "unseen_categories") if args.split_by_valid_or_test else ("members",)
    for k in need:
        if k not in members:
            raise ValueError(f"{args.members_file} has no {k!r}")
    id_dict = read_item_info(os.path.join(args.data_dir, "raw", "item_info.jsonl"))
    logger.info(f"id dict length: {len(id_dict)}")
    lines = ensemble(args, id_dict, members)

    fused, threshold, ct = [], 0.0, 0
    for d in lines.values():
        dd = copy.deepcopy(d)
        if args.ensemble_strategy == "f1":
            p = 1.0 if dd["1"] >= dd["0"] else -1.0
            ct += p > 0
        else:
            p = dd["tgt_item_emb"]
            ct += p >= threshold
        dd["tgt_item_emb"] = f"[{p}]"
        dd["threshold"] = threshold
        fused.append(dd)
    logger.info(f"p: {ct}, total: {len(fused)}")
    model_dir = os.path.join(args.data_dir, "output", "ensemble")
    os.makedirs(model_dir, exist_ok=True)
    path = os.path.join(model_dir, "deepAI_result.jsonl")
    with open(path, "w", encoding="utf-8") as w:
        for dd in fused:
            w.write(json.dumps(dd) + "\n")
    return path


if __name__ == "__main__":
    main()
