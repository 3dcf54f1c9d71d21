"""The two files finetune_graph.py reads beside the pair lists, seen from the host: the lines of processed/entity2id.txt (whose order
is the row order of processed/feature_matrix.pt, pred_text.py) and the adjacency of processed/adj_t.pt as an `edge_index`.

The reference lost the writer of adj_t.pt: the code in its data_prepare.py (:660-732) filled a dense 230 023 x 230 023 matrix and is
commented out.  build_edge_index restates what that code connected -- an item with its category value and its industry value -- and adds
the facts of the knowledge-graph split files, as a [2, E] int64 tensor models.graph.load_adjacency accepts.  No GPU is involved.
"""
import json
import os

import numpy as np
import torch

FACT_FILES = ("train2id.txt", "valid2id.txt", "test2id.txt")


def read_entity_lines(path):
    """[(entity key, id)] of an entity2id.txt (`key \\t id`), in file order; empty lines are skipped, anything else that is not
    `key \\t integer` is a ValueError naming the line."""
    out = []
    with open(path, "r", encoding="utf-8") as r:
        for no, line in enumerate(r, 1):
            line = line.strip("\n")
            if not line:
                continue
            parts = line.split("\t")
            try:
                if len(parts) != 2:
                    raise ValueError
                out.append((parts[0], int(parts[1])))
            except ValueError:
                raise ValueError(f"{path} line {no}: expected `key \\t integer id`, got {line!r}") from None
    return out


def read_item_info(path):
    """raw/item_info.jsonl as {item_id: record}, in file order"""
    info = {}
    with open(path, "r", encoding="utf-8") as r:
        for line in r:
            if line.strip():
                d = json.loads(line)
                info[d["item_id"]] = d
    return info


def build_edge_index(data_dir):
    """edge_index [2, E] int64 over the ids of processed/entity2id.txt: both directions of every edge, no duplicates, no self-loops,
    sorted by (row, column).  Edges:
      1. head <-> tail of every fact of processed/{train,valid,test}2id.txt, whichever exist (read by kg_pretrain's reader, the one
         pkgm_pretrain.py uses, so the column order `from, rel, to` cannot drift);
      2. item <-> /value/{cate_name}-{cate_id} and item <-> /value/{industry_name} for every item of raw/item_info.jsonl whose two keys
         are both in entity2id.txt (the key formats of the reference's data_prepare.py:671, :683)."""
    processed = os.path.join(data_dir, "processed")
    e2id = dict(read_entity_lines(os.path.join(processed, "entity2id.txt")))
    n_ent = max(e2id.values()) + 1 if e2id else 0
    pairs = []
    present = [f for f in FACT_FILES if os.path.isfile(os.path.join(processed, f))]
    if present:
        from ..models import kg_pretrain as K
        n_rel = K._max_id(os.path.join(processed, "relation2id.txt")) + 1
        for fname in present:
            kg = K._load_facts(processed, fname, n_ent, n_rel)
            pairs.append(np.stack((kg.head_idx.numpy(), kg.tail_idx.numpy()), axis=1))
    item_pairs = []
    for item_id, d in read_item_info(os.path.join(data_dir, "raw", "item_info.jsonl")).items():
        i = e2id.get(f"/item/{item_id}")
        if i is None:
            continue
        keys = []
        if "cate_name" in d and "cate_id" in d:
            keys.append(f"/value/{d['cate_name']}-{d['cate_id']}")
        if "industry_name" in d:
            keys.append(f"/value/{d['industry_name']}")
        item_pairs += [(i, e2id[k]) for k in keys if k in e2id]
    if item_pairs:
        pairs.append(np.asarray(item_pairs, dtype=np.int64))
    if not pairs:
        return torch.zeros((2, 0), dtype=torch.long)
    e = np.concatenate(pairs, axis=0).astype(np.int64)
    e = e[e[:, 0] != e[:, 1]]
    e = np.unique(np.concatenate((e, e[:, ::-1]), axis=0), axis=0)           # sorted by (row, column), duplicates dropped
    return torch.from_numpy(np.ascontiguousarray(e.T))
