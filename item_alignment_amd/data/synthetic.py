"""Deterministic synthetic item pairs in the tensor layouts the reference's collate functions produce
(src/data/data.py:37-74 collate_coca_pair, :172-240 collate_one_tower / collate_two_tower, :77-95
collate_image) — no dataset, tokenizer vocabulary or images exist offline.

Text: title_len ~ U{8..48}, pv_len ~ U{16..203}; ids = [CLS] title [SEP] pvs [SEP], right-padded with 0 to
max_seq_len + max_seq_len_pv (BERT-zh vocab 21128: PAD 0, CLS 101, SEP 102; draws equal to a special id are
remapped to 1000).  Images: N(0,1) fp32 NCHW (what timm's eval transform yields after mean/std).  Seed 2345
is the reference default (finetune_multimodal.py:57).
"""
import numpy as np
import torch

PAD, CLS, SEP, IMG_TOKEN = 0, 101, 102, 99
VOCAB = 21128


def _item_tokens(rs, max_title=50, max_pv=205, full_length=False):
    L = max_title + max_pv
    if full_length:
        tl, pl = max_title - 2, max_pv - 1
    else:
        tl, pl = int(rs.randint(8, max_title - 1)), int(rs.randint(16, max_pv - 1))
    body = rs.randint(1, VOCAB, size=tl + pl)
    body[np.isin(body, (PAD, IMG_TOKEN, CLS, SEP))] = 1000
    ids = np.concatenate([[CLS], body[:tl], [SEP], body[tl:], [SEP]])
    out = np.zeros(L, dtype=np.int64)
    out[:len(ids)] = ids
    return out


def two_tower_text(rs, n_pairs, max_title=50, max_pv=205, full_length=False):
    """-> dict of [n, L] int64 arrays for both towers (token_type_ids all 0, position_ids None)."""
    a = np.stack([_item_tokens(rs, max_title, max_pv, full_length) for _ in range(n_pairs)])
    b = np.stack([_item_tokens(rs, max_title, max_pv, full_length) for _ in range(n_pairs)])
    return dict(input_ids_1=a, attention_mask_1=(a != 0).astype(np.int64), token_type_ids_1=np.zeros_like(a),
                input_ids_2=b, attention_mask_2=(b != 0).astype(np.int64), token_type_ids_2=np.zeros_like(b))


def one_tower_text(rs, n_pairs, max_title=50, max_pv=205, full_length=False):
    """[CLS] src [SEP] src_pv [SEP] tgt [SEP] tgt_pv [SEP] padded to 2*(max_title+max_pv); segment ids 0 / 1
    (what tokenizer(text, text_pair, max_length=2L, padding=max_length) yields, reference data.py:558-559)."""
    L = 2 * (max_title + max_pv)
    ids = np.zeros((n_pairs, L), dtype=np.int64)
    tt = np.zeros((n_pairs, L), dtype=np.int64)
    for i in range(n_pairs):
        a = _item_tokens(rs, max_title, max_pv, full_length)
        b = _item_tokens(rs, max_title, max_pv, full_length)
        a, b = a[a != 0], b[b != 0][1:]               # second segment has no [CLS]
        ids[i, :len(a)] = a
        ids[i, len(a):len(a) + len(b)] = b
        tt[i, len(a):len(a) + len(b)] = 1
    return dict(input_ids=ids, attention_mask=(ids != 0).astype(np.int64), token_type_ids=tt)


class SyntheticCocaPairs:
    """Batches for CoCaForItemAlignment in collate_coca_pair order (reference data.py:73-74, after the two id lists):
    input_ids_1, attention_mask_1, token_type_ids_1, position_ids_1, images_1, ..._2, labels."""

    def __init__(self, n_pairs, image_size=384, max_title=50, max_pv=205, seed=2345, full_length=False):
        rs = np.random.RandomState(seed)
        self.text = two_tower_text(rs, n_pairs, max_title, max_pv, full_length)
        self.labels = rs.randint(0, 2, size=n_pairs).astype(np.int64)
        self.n, self.image_size, self.seed = n_pairs, image_size, seed

    def batch(self, indices, device, device_images=False):
        """device_images: draw the N(0,1) images with the device's generator (fast for many large resident batches; a different
        stream than the host generator, still a function of (seed, first index) only)."""
        idx = np.asarray(indices)
        t = {k: torch.from_numpy(v[idx]).to(device) for k, v in self.text.items()}
        S = self.image_size
        if device_images and torch.device(device).type == "cuda":
            g = torch.Generator(device=device).manual_seed(self.seed * 7919 + int(idx[0]))
            im1 = torch.randn((len(idx), 3, S, S), generator=g, device=device)
            im2 = torch.randn((len(idx), 3, S, S), generator=g, device=device)
        else:
            g = torch.Generator(device="cpu").manual_seed(self.seed * 7919 + int(idx[0]))
            im1 = torch.randn((len(idx), 3, S, S), generator=g).to(device)
            im2 = torch.randn((len(idx), 3, S, S), generator=g).to(device)
        labels = torch.from_numpy(self.labels[idx]).to(device)
        # PairedMultimodalDataset emits explicit position ids 0..L-1 (reference data.py:979,984)
        pos = torch.arange(t["input_ids_1"].shape[1], device=device).unsqueeze(0).expand(len(idx), -1).contiguous()
        return (t["input_ids_1"], t["attention_mask_1"], t["token_type_ids_1"], pos, im1,
                t["input_ids_2"], t["attention_mask_2"], t["token_type_ids_2"], pos, im2, labels)


class SyntheticItemGraph:
    """A bipartite item / attribute-value graph for the graph two-tower model (finetune_graph.py), the shape the commented-out
    lines of the reference's data_prepare.py:690-704 built: nodes 0 .. n_items-1 are items, the rest values; a symmetric 0/1
    adjacency with an edge both ways between an item and each of its values.  Item degree ~ U{5..40}; value popularity is
    Zipf-like (p ~ 1 / (rank + 50)), so a few value nodes reach degrees in the thousands on a large graph.  Items come in twins: item
    2k+1 re-uses about 70 % of the values of item 2k.  Features are N(0,1) fp32.  A pair's label is a function of the shared
    neighbours alone: 1 iff the two items share at least 40 % of the smaller value set."""

    def __init__(self, n_items, n_values, seed=2345, feature_dim=64, n_pairs=None):
        rs = np.random.RandomState(seed)
        self.n_items, self.n_values, self.seed, self.feature_dim = int(n_items), int(n_values), seed, int(feature_dim)
        pop = 1.0 / (np.arange(n_values) + 50.0)
        pop /= pop.sum()
        degs = np.minimum(rs.randint(5, 41, size=n_items), n_values)
        draws = rs.choice(n_values, size=int(degs.sum()), replace=True, p=pop)      # one draw for every item (a per-item call is O(n_values))
        ends = np.cumsum(degs)
        keep_u = rs.rand(n_items, 40)
        self.item_values = []
        for i in range(n_items):
            fresh = draws[ends[i] - degs[i]:ends[i]]
            if i % 2 == 1:
                twin = self.item_values[i - 1]
                keep = twin[keep_u[i, :len(twin)] < 0.7]
                vals = np.unique(np.concatenate([keep, fresh]))[:max(int(degs[i]), len(keep))]
            else:
                vals = np.unique(fresh)
            self.item_values.append(vals.astype(np.int64))
        self.num_nodes = n_items + n_values
        src = np.concatenate([np.full(len(v), i, np.int64) for i, v in enumerate(self.item_values)])
        dst = np.concatenate(self.item_values) + n_items
        self.edge_index = torch.from_numpy(np.stack([np.concatenate([src, dst]), np.concatenate([dst, src])]))
        self.features = torch.from_numpy(rs.standard_normal((self.num_nodes, feature_dim)).astype(np.float32))
        n_pairs = int(n_pairs if n_pairs is not None else n_items)
        a = rs.randint(0, n_items, size=n_pairs)
        b = np.where(rs.rand(n_pairs) < 0.5, a ^ 1, rs.randint(0, n_items, size=n_pairs))
        b = np.minimum(b, n_items - 1)
        self.pairs = [self.pair(int(x), int(y)) for x, y in zip(a, b)]

    @property
    def nnz(self):
        return int(self.edge_index.shape[1])

    def label(self, a, b):
        va, vb = self.item_values[a], self.item_values[b]
        return int(len(np.intersect1d(va, vb)) >= 0.4 * min(len(va), len(vb)))

    def pair(self, a, b):
        return {"src_item_id": f"item{a}", "tgt_item_id": f"item{b}", "src_idx": a, "tgt_idx": b, "item_label": str(self.label(a, b))}

    def adjacency(self):
        """torch sparse COO [N, N] fp32 of ones."""
        return torch.sparse_coo_tensor(self.edge_index, torch.ones(self.nnz), (self.num_nodes, self.num_nodes)).coalesce()

    def write(self, data_dir, splits=(0.6, 0.2, 0.2)):
        """The input files of finetune_graph.py under data_dir: processed/entity2id.txt, processed/adj_t.pt,
        processed/feature_matrix.pt, raw/item_train_train_pair.jsonl, raw/item_train_valid_pair.jsonl, raw/item_valid_pair.jsonl
        (the last without labels, like the reference's test file)."""
        import json
        import os
        os.makedirs(os.path.join(data_dir, "processed"), exist_ok=True)
        os.makedirs(os.path.join(data_dir, "raw"), exist_ok=True)
        with open(os.path.join(data_dir, "processed", "entity2id.txt"), "w", encoding="utf-8") as w:
            for i in range(self.n_items):
                w.write(f"/item/item{i}\t{i}\n")
            for v in range(self.n_values):
                w.write(f"/value/v{v}\t{self.n_items + v}\n")
        torch.save(self.adjacency(), os.path.join(data_dir, "processed", "adj_t.pt"))
        torch.save(self.features, os.path.join(data_dir, "processed", "feature_matrix.pt"))
        n = len(self.pairs)
        n_train, n_valid = int(n * splits[0]), int(n * splits[1])
        parts = {"item_train_train_pair.jsonl": self.pairs[:n_train], "item_train_valid_pair.jsonl": self.pairs[n_train:n_train + n_valid],
                 "item_valid_pair.jsonl": self.pairs[n_train + n_valid:]}
        for name, rows in parts.items():
            with open(os.path.join(data_dir, "raw", name), "w", encoding="utf-8") as w:
                for r in rows:
                    d = {k: r[k] for k in ("src_item_id", "tgt_item_id")}
                    if name != "item_valid_pair.jsonl":
                        d["item_label"] = r["item_label"]
                    w.write(json.dumps(d) + "\n")
        return parts
