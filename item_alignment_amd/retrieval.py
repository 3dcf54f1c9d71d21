"""Same-item retrieval over a catalogue of embeddings: for every query row its k most similar catalogue rows by cosine or inner product,
exact brute force on the bf16 matrix cores (csrc/simtopk.hip: ia_sim_rows_bf16, ia_sim_topk), without an N x N score matrix.

    prepare_rows   fp32 rows -> the bf16 rows the scan reads (zero-padded to the row pitch, optionally L2-normalised)
    sim_topk       one ia_sim_topk call
    ItemIndex      a prepared catalogue on the GPU; .search() batches the queries; .from_file() reads feature_matrix.pt + entity2id.txt
                   (pred_text.py), image_embedding.json (image_embedding.py) or a two-tower deepAI_result_*.jsonl (--do_pred)
    recall_at_k    recall and mean reciprocal rank of labelled positive pairs in the neighbour lists

There is no CPU path: the kernels are the only implementation (loading and the recall are host code and need no GPU).
"""
import json

import torch

from . import _lib
from ._lib import check, stream_ptr

F32, BF16 = torch.float32, torch.bfloat16
TOPK_MAX_K = 64      # IA_SIM_TOPK_MAX_K
METRICS = ("cosine", "ip")


def row_pitch(D):
    """elements per prepared row"""
    return int(_lib.load().ia_sim_row_pitch(int(D)))


def prepare_rows(x, normalize):
    """x: fp32 [rows, D] on the GPU (any row stride, unit column stride) -> bf16 [rows, pitch]: bf16(x * inv), inv = 1 or
    1 / max(|row|_2, 1e-12); the pad columns are zero."""
    if x.dim() != 2 or x.dtype != F32 or not x.is_cuda:
        raise ValueError(f"prepare_rows takes an fp32 [rows, D] tensor on the GPU, got {x.dtype} {tuple(x.shape)} on {x.device}")
    rows, D = x.shape
    if D < 1:
        raise ValueError("prepare_rows: rows of width 0")
    if x.stride(1) != 1 or (rows > 1 and x.stride(0) < D):
        x = x.contiguous()
    out = torch.empty(rows, row_pitch(D), device=x.device, dtype=BF16)
    if rows:
        check(_lib.load().ia_sim_rows_bf16(x.data_ptr(), x.stride(0) if rows > 1 else D, rows, D, 1 if normalize else 0, out.data_ptr(),
                                           stream_ptr()), "ia_sim_rows_bf16")
    return out


def sim_topk(q, cand, D, k, skip=None, max_splits=0, workspace=None):
    """One ia_sim_topk call.  q [B, pitch], cand [n_cand, pitch]: prepared bf16 rows of width D.  skip: int64 [B], the candidate each
    query never gets back (-1: none).  Returns (idx int64 [B, k], score fp32 [B, k]) on the device, best first in the order (score
    descending, candidate index ascending); unused slots hold -1 / -inf."""
    lib = _lib.load()
    pitch = row_pitch(D)
    for name, t in (("q", q), ("cand", cand)):
        if t.dim() != 2 or t.dtype != BF16 or not t.is_cuda or t.shape[1] != pitch or not t.is_contiguous():
            raise ValueError(f"{name} must be contiguous prepared bf16 rows [n, {pitch}] on the GPU (prepare_rows), got {t.dtype} "
                             f"{tuple(t.shape)} on {t.device}")
    if not 1 <= k <= TOPK_MAX_K:
        raise ValueError(f"k must lie in [1, {TOPK_MAX_K}], got {k}")
    B, n_cand = q.shape[0], cand.shape[0]
    dev = q.device
    idx = torch.full((B, k), -1, device=dev, dtype=torch.int64)
    score = torch.full((B, k), float("-inf"), device=dev, dtype=F32)
    if B == 0 or n_cand == 0:
        return idx, score
    if skip is not None:
        skip = torch.as_tensor(skip, dtype=torch.int64).to(dev).contiguous()
        if skip.shape != (B,):
            raise ValueError(f"skip must hold one candidate index per query, got {tuple(skip.shape)} for {B} queries")
    nbytes = lib.ia_sim_topk_workspace_bytes(B, D, n_cand, k, max_splits)
    if workspace is None or workspace.numel() < nbytes:
        workspace = torch.empty(max(nbytes, 1), device=dev, dtype=torch.uint8)
    check(lib.ia_sim_topk(q.data_ptr(), cand.data_ptr(), B, D, n_cand, None if skip is None else skip.data_ptr(), k, max_splits,
                          idx.data_ptr(), score.data_ptr(), workspace.data_ptr(), workspace.numel(), stream_ptr()), "ia_sim_topk")
    return idx, score


# ------------------------------------------------------------------------------------------------ loaders (host)
def _parse_vec(text, where):
    try:
        v = json.loads(text) if isinstance(text, str) else text
        v = [float(a) for a in v]
    except (TypeError, ValueError):
        raise ValueError(f"{where}: not a list of numbers: {str(text)[:60]!r}")
    return v


def _stack(ids, rows, where_of):
    """rows of one length >= 2 -> fp32 [N, D]; `where_of(i)` names row i in a message"""
    if not rows:
        raise ValueError("no embeddings found")
    D = len(rows[0])
    for i, r in enumerate(rows):
        if len(r) != D:
            raise ValueError(f"{where_of(i)}: a row of {len(r)} numbers, the rows before it have {D}")
    if D < 2:
        raise ValueError(f"{where_of(0)}: rows of {D} number(s) are no embeddings (a one-tower prediction file holds probabilities)")
    return list(ids), torch.tensor(rows, dtype=F32)


def load_pt(path, ids_file=None):
    x = torch.load(path, map_location="cpu")
    if not torch.is_tensor(x) or x.dim() != 2:
        raise ValueError(f"{path}: a [N, D] tensor is expected")
    if x.shape[1] < 2:
        raise ValueError(f"{path}: rows of {x.shape[1]} number(s) are no embeddings")
    x = x.to(F32)
    if ids_file is None:
        return [str(i) for i in range(x.shape[0])], x, 0
    ids = []
    with open(ids_file, "r", encoding="utf-8") as f:
        for line in f:
            if line.strip():
                ids.append(line.rstrip("\n").split("\t")[0])
    if len(ids) != x.shape[0]:
        raise ValueError(f"{ids_file}: {len(ids)} ids for the {x.shape[0]} rows of {path}")
    return ids, x, 0


def load_json(path):
    with open(path, "r", encoding="utf-8") as f:
        obj = json.load(f)
    if not isinstance(obj, dict):
        raise ValueError(f"{path}: one object mapping item id to a list of floats is expected")
    ids = list(obj)
    rows = [_parse_vec(obj[i], f"{path} item {i}") for i in ids]
    ids, x = _stack(ids, rows, lambda i: f"{path} item {ids[i]}")
    return ids, x, 0


def load_jsonl(path):
    """A two-tower prediction file: the first occurrence of an item id wins; returns also the number of later occurrences that differ."""
    seen, ids, rows, lines, differing = {}, [], [], [], 0
    with open(path, "r", encoding="utf-8") as f:
        for no, line in enumerate(f, 1):
            if not line.strip():
                continue
            try:
                rec = json.loads(line)
            except ValueError:
                raise ValueError(f"{path} line {no}: not a JSON object")
            for side in ("src", "tgt"):
                try:
                    item, emb = str(rec[f"{side}_item_id"]), rec[f"{side}_item_emb"]
                except (KeyError, TypeError):
                    raise ValueError(f"{path} line {no}: no {side}_item_id / {side}_item_emb")
                v = _parse_vec(emb, f"{path} line {no} {side}_item_emb")
                if item in seen:
                    differing += rows[seen[item]] != v
                    continue
                seen[item] = len(ids)
                ids.append(item)
                rows.append(v)
                lines.append(no)
    ids, x = _stack(ids, rows, lambda i: f"{path} line {lines[i]}")
    return ids, x, differing


def load_embeddings(path, ids_file=None):
    """(ids, fp32 [N, D], differing) by the file's suffix: .pt (+ ids_file), .json, .jsonl"""
    p = str(path)
    if p.endswith(".pt"):
        return load_pt(p, ids_file)
    if p.endswith(".jsonl"):
        return load_jsonl(p)
    if p.endswith(".json"):
        return load_json(p)
    raise ValueError(f"{path}: unknown embedding format (use .pt, .json or .jsonl)")


# ------------------------------------------------------------------------------------------------ the index
class ItemIndex:
    """A catalogue of N embeddings prepared for ia_sim_topk and held on the GPU.  ids: one label per row (default: the row number)."""

    def __init__(self, embeddings, ids=None, metric="cosine", keep_fp32=True, device=None):
        if metric not in METRICS:
            raise ValueError(f"metric {metric!r}: use 'cosine' or 'ip'")
        x = torch.as_tensor(embeddings)
        if x.dim() != 2 or x.shape[1] < 1:
            raise ValueError(f"embeddings must be [N, D], got {tuple(x.shape)}")
        self.metric, self.N, self.D = metric, x.shape[0], x.shape[1]
        self.ids = list(range(self.N)) if ids is None else list(ids)
        if len(self.ids) != self.N:
            raise ValueError(f"{len(self.ids)} ids for {self.N} rows")
        if not torch.cuda.is_available():
            raise RuntimeError("ItemIndex runs on the GPU (HIP kernels, no CPU path)")
        self.device = torch.device(device or "cuda")
        self.differing = 0
        self.rows = self._prepare(x)                          # bf16 [N, pitch] on the GPU
        self.fp32 = self._fp32(x) if keep_fp32 else None      # fp32 (normalised) rows on the host, for rescore
        self._ws = None

    @classmethod
    def from_file(cls, path, ids_file=None, metric="cosine", **kw):
        ids, x, differing = load_embeddings(path, ids_file)
        index = cls(x, ids, metric, **kw)
        index.differing = differing
        return index

    def _fp32(self, x):
        x = x.detach().to("cpu", F32)
        return torch.nn.functional.normalize(x, dim=1, eps=1e-12) if self.metric == "cosine" else x

    def _prepare(self, x, chunk=65536):
        out = torch.empty(x.shape[0], row_pitch(self.D), device=self.device, dtype=BF16)
        for lo in range(0, x.shape[0], chunk):
            out[lo:lo + chunk] = prepare_rows(x[lo:lo + chunk].detach().to(self.device, F32), self.metric == "cosine")
        return out

    def search(self, queries=None, k=10, batch_size=4096, exclude_self=None, rescore=False):
        """(idx int64 [B, k], score fp32 [B, k]) on the CPU: for every query row the catalogue ROW NUMBERS of its k best rows (-1 / -inf
        in unused slots).  queries=None: every catalogue row queries the catalogue, and a row is kept out of its own list unless
        exclude_self=False.  With foreign queries exclude_self=True keeps catalogue row i from query i.  rescore: the scores of the
        returned rows recomputed as fp32 dots of the fp32 (normalised) rows and each list re-sorted by them (which rows are returned
        does not change)."""
        if not 1 <= k <= TOPK_MAX_K:
            raise ValueError(f"k must lie in [1, {TOPK_MAX_K}], got {k}")
        if batch_size < 1:
            raise ValueError(f"batch_size must be positive, got {batch_size}")
        own = queries is None
        if exclude_self is None:
            exclude_self = own
        if own:
            qrows, qf = self.rows, self.fp32
        else:
            q = torch.as_tensor(queries)
            if q.dim() != 2 or q.shape[1] != self.D:
                raise ValueError(f"queries must be [B, {self.D}], got {tuple(q.shape)}")
            qrows, qf = self._prepare(q), (self._fp32(q) if rescore else None)
        if rescore and self.fp32 is None:
            raise ValueError("rescore needs the fp32 rows: build the index with keep_fp32=True")
        B = qrows.shape[0]
        idx = torch.empty(B, k, dtype=torch.int64)
        score = torch.empty(B, k, dtype=F32)
        for lo in range(0, B, batch_size):
            hi = min(B, lo + batch_size)
            skip = torch.arange(lo, hi, dtype=torch.int64, device=self.device) if exclude_self else None
            nbytes = _lib.load().ia_sim_topk_workspace_bytes(hi - lo, self.D, self.N, k, 0)
            if self._ws is None or self._ws.numel() < nbytes:
                self._ws = torch.empty(max(nbytes, 1), device=self.device, dtype=torch.uint8)
            i, s = sim_topk(qrows[lo:hi], self.rows, self.D, k, skip=skip, workspace=self._ws)
            idx[lo:hi], score[lo:hi] = i.cpu(), s.cpu()
        if rescore:
            idx, score = self._rescore(idx, score, qf)
        return idx, score

    def _rescore(self, idx, score, qf, chunk=1024):
        used = idx >= 0
        for lo in range(0, idx.shape[0], chunk):
            rows = self.fp32[idx[lo:lo + chunk].clamp(min=0)]                        # [b, k, D]
            s = (rows * qf[lo:lo + chunk, None, :]).sum(-1)
            score[lo:lo + chunk] = torch.where(used[lo:lo + chunk], s, score[lo:lo + chunk])
        # (score descending, row number ascending) inside each list: a stable sort by score of the lists put in row order
        by_id = torch.where(used, idx, torch.full_like(idx, torch.iinfo(torch.int64).max)).argsort(dim=1, stable=True)
        idx, score = idx.gather(1, by_id), score.gather(1, by_id)
        by_score = (-score).argsort(dim=1, stable=True)
        return idx.gather(1, by_score), score.gather(1, by_score)


def recall_at_k(idx, ids, pairs, query_ids=None):
    """idx [B, k]: the lists of ItemIndex.search (catalogue row numbers), query row b being item query_ids[b] (default: ids[b], the
    catalogue queried itself).  pairs: (src_item_id, tgt_item_id, item_label).  Over the pairs with label 1 whose src is a query and
    whose tgt is in the catalogue: (the share whose tgt is in src's list, the mean of 1 / rank with 0 where absent, their number, the
    number of label-1 pairs left out because an id is unknown)."""
    def first_row(labels):
        rows = {}
        for n, i in enumerate(labels):
            rows.setdefault(str(i), n)
        return rows
    row_of = first_row(ids)
    q_of = row_of if query_ids is None else first_row(query_ids)
    lists = idx.tolist()
    hits, rr, used, skipped = 0, 0.0, 0, 0
    for src, tgt, label in pairs:
        if int(label) != 1:
            continue
        qs, t = q_of.get(str(src)), row_of.get(str(tgt))
        if qs is None or t is None:
            skipped += 1
            continue
        used += 1
        if t in lists[qs]:
            hits += 1
            rr += 1.0 / (lists[qs].index(t) + 1)
    return (hits / used if used else 0.0), (rr / used if used else 0.0), used, skipped
