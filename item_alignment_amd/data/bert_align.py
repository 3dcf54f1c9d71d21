"""Data layer of the BERT pair classifier (reference src/bert/data_utils.py), restated: the pair file is read once per field, every
field of a pair is tokenised as a sentence pair padded to that field's own length, and the loader yields the sixteen tensors
finetune_bert.py / pred_bert.py unpack -- ids, mask, token types of pvs, title, cate, cate_path, industry_name, then the label.

The one change: the pvs shuffle (`;`-separated attributes reordered, the two sides swapped half of the time) draws from a generator
seeded by the caller, not from the global `random` / numpy state, so a run is reproducible from its --seed alone.
"""
import json
import logging
import os
import random

import torch
from torch.utils.data import DataLoader, RandomSampler, SequentialSampler, TensorDataset

LOGGER = logging.getLogger("bert_align")

FIELD_PAIRS = (("pvs_a", "pvs_b"), ("title_a", "title_b"), ("industry_name_a", "industry_name_b"), ("cate_a", "cate_b"),
               ("cate_path_a", "cate_path_b"))


def read_data(data_dir, file, pair_names):
    """[[record[pair_names[0]], record[pair_names[1]], int(label)], ...] of a JSON list of records, or of {"data": [...]}; a field a
    record lacks is the empty string"""
    with open(os.path.join(data_dir, file), "r", encoding="utf8") as f:
        data = json.load(f)
    if isinstance(data, dict) and "data" in data:
        data = data["data"]
    a, b = pair_names
    return [[rec.get(a, ""), rec.get(b, ""), int(rec["label"])] for rec in data]


def shuffle_pvs_pairs(pvs_pairs, seed=0):
    """every side's `;`-separated attributes in a random order, and the two sides swapped with probability one half"""
    rng = random.Random(seed)
    out = []
    for pvs_a, pvs_b, label in pvs_pairs:
        parts_a, parts_b = pvs_a.split(";"), pvs_b.split(";")
        rng.shuffle(parts_a)
        rng.shuffle(parts_b)
        a, b = ";".join(parts_a), ";".join(parts_b)
        out.append([b, a, label] if rng.random() < 0.5 else [a, b, label])
    return out


def join_data(data_dir, filename, do_shuffle=True, seed=0):
    """-> pvs, title, industry_name, cate, cate_path pair lists (the reference's order)"""
    pvs, title, industry_name, cate, cate_path = (read_data(data_dir, filename, list(names)) for names in FIELD_PAIRS)
    if do_shuffle:
        pvs = shuffle_pvs_pairs(pvs, seed)
    return pvs, title, industry_name, cate, cate_path


def show(data, mode, name, show_num=3):
    LOGGER.info(f"======= {mode} / {name} ==========")
    for row in data[:show_num]:
        LOGGER.info(row)


def show_pairs(src_data, tgt_data, labels, name, mode="train", show_num=3):
    LOGGER.info(f"======= {mode} / {name} ==========")
    for a, b, label in zip(src_data[:show_num], tgt_data[:show_num], labels[:show_num]):
        LOGGER.info(f"src_{name}:{a}")
        LOGGER.info(f"tgt_{name}:{b}")
        LOGGER.info(f"label:{label}")


def get_examples(pvs, titles, cates, cate_paths, industry_names):
    """the pair lists as columns: (pvs_src, pvs_tgt, titles_src, titles_tgt, cate_src, cate_tgt, cate_path_src, cate_path_tgt,
    industry_name_src, industry_name_tgt, labels), each a tuple over the pairs"""
    cols = []
    labels = ()
    for pairs in (pvs, titles, cates, cate_paths, industry_names):
        src, tgt, labels = zip(*pairs)
        cols += [src, tgt]
    return (*cols, labels)


def encode(tokenizer, pvs_src, pvs_tgt, title_src, title_tgt, cate_src, cate_tgt, cate_path_src, cate_path_tgt, industry_name_src,
           industry_name_tgt, pvs_len=512, title_len=150, cate_len=20, cate_path_len=50, industry_name_len=20):
    """-> pvs, title, cate, cate_path, industry_name encodings: [CLS] a [SEP] b [SEP], truncated (longest side first) and padded to the
    field's length"""
    def enc(src, tgt, n, name):
        out = tokenizer(list(src), list(tgt), padding="max_length", truncation=True, max_length=n)
        LOGGER.info(f"{name} encoded")
        return out
    return (enc(pvs_src, pvs_tgt, pvs_len, "pvs"), enc(title_src, title_tgt, title_len, "title"), enc(cate_src, cate_tgt, cate_len, "cate"),
            enc(cate_path_src, cate_path_tgt, cate_path_len, "cate_path"),
            enc(industry_name_src, industry_name_tgt, industry_name_len, "industry_name"))


def get_dataloader(pvs, titles, cates, cate_paths, industry_names, labels, batch_size=4, mode="train", generator=None):
    """A loader over TensorDataset(ids, mask, token types of pvs, title, cate, cate_path, industry_name; labels): sixteen int64
    tensors.  mode "train": a random order, from `generator` when one is given (not in the reference: finetune_bert.py seeds it per
    epoch); any other mode: file order."""
    tensors = []
    for e in (pvs, titles, cates, cate_paths, industry_names):
        tensors += [torch.tensor(e["input_ids"]), torch.tensor(e["attention_mask"]), torch.tensor(e["token_type_ids"])]
    data = TensorDataset(*tensors, torch.tensor(labels))
    sampler = RandomSampler(data, generator=generator) if mode == "train" else SequentialSampler(data)
    return DataLoader(data, sampler=sampler, batch_size=batch_size)


# ---------------------------------------------------------------------------------------------- evaluation arithmetic (host)
def find_best_f1_and_threshold(scores, labels, high_score_more_similar=True):
    """The cut of the score-sorted pairs with the best F1 -> (accuracy, F1, precision, recall, threshold).  As the reference
    (finetune_bert.py:72-106): the cut behind the LAST row is never tried ("everything is a match" is not a candidate), and the
    threshold is the mid-point between the last row kept and the first one dropped."""
    assert len(scores) == len(labels)
    rows = sorted(zip(scores, labels), key=lambda r: r[0], reverse=high_score_more_similar)
    positives = sum(labels)
    negatives = len(labels) - positives
    best = (0, 0, 0, 0, 0)
    kept = hits = 0
    for i in range(len(rows) - 1):
        kept += 1
        hits += 1 if rows[i][1] == 1 else 0
        if hits == 0:
            continue
        precision, recall = hits / kept, hits / positives
        f1 = 2 * precision * recall / (precision + recall)
        if f1 > best[1]:
            acc = (hits + negatives - (kept - hits)) / len(labels)
            best = (acc, f1, precision, recall, (rows[i][0] + rows[i + 1][0]) / 2)
    return best


def confusion(logits, labels):
    """argmax counts over [N, 2] logits -> tp, fp, tn, fn"""
    tp = fp = tn = fn = 0
    for row, t in zip(logits, labels):
        p = 1 if row[1] > row[0] else 0       # numpy's argmax: the first of equal logits
        if p == t:
            tp, tn = tp + (t == 1), tn + (t == 0)
        else:
            fn, fp = fn + (t == 1), fp + (t == 0)
    return tp, fp, tn, fn


def pred_probability(weight, bias, pool_out):
    """(score, p) of pred_bert.py, literally: score = w . pool_out + b, p = 1 / (1 + exp(-score - b)).  The bias enters twice (the
    reference's `threshold = -bias` is added to a score that already holds the bias): kept, a quirk of the reference."""
    import math
    score = float((weight * pool_out).sum() + bias)
    return score, 1.0 / (1.0 + math.exp(-score + (-float(bias))))
