"""Same-item retrieval over a catalogue of embeddings: for every query row its k most similar catalogue rows by cosine or inner product,
exact brute force on the bf16 matrix cores (csrc/simtopk.hip: ia_sim_rows_bf16, ia_sim_topk), without an N x N score matrix.

    prepare_rows   fp32 rows -> the bf16 rows the scan reads (zero-padded to the row pitch, optionally L2-normalised)
    sim_topk       one ia_sim_topk call
    ItemIndex      a prepared catalogue on the GPU; .search() batches the queries; .from_file() reads feature_matrix.pt + entity2id.txt
                   (pred_text.py), image_embedding.json (image_embedding.py) or a two-tower deepAI_result_*.jsonl (--do_pred)
    IVFItemIndex   the same catalogue behind an inverted-file index (csrc/simtopk_groups.hip): spherical k-means centroids partition it
                   into lists and a query scans only the nprobe lists whose centroids are most similar to it -- approximate, sub-quadratic
    sim_topk_groups, sim_topk_fold, centroid_sums   one call of ia_sim_topk_groups / ia_sim_topk_fold / ia_sim_centroid_sums
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


def _offsets(counts):
    """int64 [n + 1] offsets of the int64 [n] counts, on their device"""
    off = torch.zeros(counts.numel() + 1, device=counts.device, dtype=torch.int64)
    off[1:] = counts.cumsum(0)
    return off


def sim_topk_groups(q, cand, q_off, c_off, D, k, label=None, skip=None, max_splits=0, workspace=None, covered=False):
    """One ia_sim_topk_groups call: group g pairs the rows [q_off[g], q_off[g + 1]) of q with the rows [c_off[g], c_off[g + 1]) of cand
    (prepared bf16 rows; the offsets int64 [G + 1], non-decreasing).  label: int32 / int64 [n_cand], the id reported for a candidate row
    (default: its position); skip: int64 [P], the candidate POSITION each query row never gets back (-1: none).  Returns (idx int64
    [P, k], score fp32 [P, k]) on the device, each row best first in (score descending, reported id ascending); unused slots, and the
    rows of no group, hold -1 / -inf.  covered: the caller states that every row of q belongs to a group (q_off[0] = 0, q_off[G] = P),
    so the kernels write every row and the outputs are not filled first."""
    lib = _lib.load()
    pitch = row_pitch(D)
    for name, t in (("q", q), ("cand", cand)):
        if t.dim() != 2 or t.dtype != BF16 or not t.is_cuda or t.shape[1] != pitch or not t.is_contiguous():
            raise ValueError(f"{name} must be contiguous prepared bf16 rows [n, {pitch}] on the GPU (prepare_rows), got {t.dtype} "
                             f"{tuple(t.shape)} on {t.device}")
    if not 1 <= k <= TOPK_MAX_K:
        raise ValueError(f"k must lie in [1, {TOPK_MAX_K}], got {k}")
    dev = q.device
    q_off, c_off = (torch.as_tensor(o, dtype=torch.int64).to(dev).contiguous() for o in (q_off, c_off))
    if q_off.dim() != 1 or q_off.shape != c_off.shape or q_off.numel() < 1:
        raise ValueError(f"q_off and c_off must hold G + 1 offsets each, got {tuple(q_off.shape)} and {tuple(c_off.shape)}")
    P, n_cand, G = q.shape[0], cand.shape[0], q_off.numel() - 1
    if covered and P and G:
        idx = torch.empty(P, k, device=dev, dtype=torch.int64)
        score = torch.empty(P, k, device=dev, dtype=F32)
    else:
        idx = torch.full((P, k), -1, device=dev, dtype=torch.int64)
        score = torch.full((P, k), float("-inf"), device=dev, dtype=F32)
    if P == 0 or G == 0:
        return idx, score
    bits = 0
    if label is not None:
        label = label.to(dev).contiguous()
        if label.dtype not in (torch.int32, torch.int64) or label.shape != (n_cand,):
            raise ValueError(f"label must be int32 or int64 [{n_cand}], got {label.dtype} {tuple(label.shape)}")
        bits = 32 if label.dtype == torch.int32 else 64
    if skip is not None:
        skip = torch.as_tensor(skip, dtype=torch.int64).to(dev).contiguous()
        if skip.shape != (P,):
            raise ValueError(f"skip must hold one candidate position per query row, got {tuple(skip.shape)} for {P} rows")
    nbytes = lib.ia_sim_topk_groups_workspace_bytes(P, G, D, n_cand, k, max_splits)
    if workspace is None or workspace.numel() < nbytes:
        workspace = torch.empty(max(nbytes, 1), device=dev, dtype=torch.uint8)
    check(lib.ia_sim_topk_groups(q.data_ptr(), cand.data_ptr(), q_off.data_ptr(), c_off.data_ptr(), G, P, D, n_cand,
                                 None if label is None else label.data_ptr(), bits, None if skip is None else skip.data_ptr(), k, max_splits,
                                 idx.data_ptr(), score.data_ptr(), workspace.data_ptr(), workspace.numel(), stream_ptr()), "ia_sim_topk_groups")
    return idx, score


def sim_topk_fold(idx_in, score_in, rows_of):
    """One ia_sim_topk_fold call.  idx_in / score_in: [P, k] as sim_topk_groups returns them; rows_of: int64 [B, nprobe], the rows whose
    lists belong to query b (-1: none; no id twice among them).  Returns (idx int64 [B, k], score fp32 [B, k]) on the device."""
    P, k = idx_in.shape
    if idx_in.dtype != torch.int64 or score_in.dtype != F32 or score_in.shape != idx_in.shape or not idx_in.is_cuda:
        raise ValueError(f"idx_in / score_in must be int64 / fp32 [P, k] on the GPU, got {idx_in.dtype} {tuple(idx_in.shape)}, "
                         f"{score_in.dtype} {tuple(score_in.shape)}")
    rows_of = torch.as_tensor(rows_of, dtype=torch.int64).to(idx_in.device).contiguous()
    if rows_of.dim() != 2 or rows_of.shape[1] < 1:
        raise ValueError(f"rows_of must be [B, nprobe], got {tuple(rows_of.shape)}")
    B, nprobe = rows_of.shape
    idx = torch.empty(B, k, device=idx_in.device, dtype=torch.int64)
    score = torch.empty(B, k, device=idx_in.device, dtype=F32)
    idx_in, score_in = idx_in.contiguous(), score_in.contiguous()
    check(_lib.load().ia_sim_topk_fold(idx_in.data_ptr(), score_in.data_ptr(), P, rows_of.data_ptr(), B, nprobe, k, idx.data_ptr(),
                                       score.data_ptr(), stream_ptr()), "ia_sim_topk_fold")
    return idx, score


def centroid_sums(rows, D, order, list_off):
    """One ia_sim_centroid_sums call.  rows: prepared bf16 [n, pitch]; order: int64 row numbers, the rows sorted by list; list_off: int64
    [nlist + 1] into order.  Returns (sums fp32 [nlist, D], counts int64 [nlist]) on the device; a list's rows are added in `order`."""
    if rows.dim() != 2 or rows.dtype != BF16 or not rows.is_cuda or rows.shape[1] != row_pitch(D) or not rows.is_contiguous():
        raise ValueError(f"rows must be contiguous prepared bf16 rows [n, {row_pitch(D)}] on the GPU, got {rows.dtype} {tuple(rows.shape)}")
    dev = rows.device
    order, list_off = (torch.as_tensor(o, dtype=torch.int64).to(dev).contiguous() for o in (order, list_off))
    nlist = list_off.numel() - 1
    if order.dim() != 1 or list_off.dim() != 1 or nlist < 0:
        raise ValueError(f"order must be [n] and list_off [nlist + 1], got {tuple(order.shape)} and {tuple(list_off.shape)}")
    sums = torch.empty(nlist, D, device=dev, dtype=F32)
    counts = torch.empty(nlist, device=dev, dtype=torch.int64)
    check(_lib.load().ia_sim_centroid_sums(rows.data_ptr(), rows.shape[0], D, order.data_ptr(), order.numel(), list_off.data_ptr(), nlist,
                                           sums.data_ptr(), counts.data_ptr(), stream_ptr()), "ia_sim_centroid_sums")
    return sums, counts


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
class _Index:
    """What the exact and the inverted-file index share: the checks of the constructor and of search(), row preparation, rescore."""

    def _setup(self, embeddings, ids, metric, device):
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
            raise RuntimeError(f"{type(self).__name__} runs on the GPU (HIP kernels, no CPU path)")
        self.device = torch.device(device or "cuda")
        self.differing = 0
        self._ws = None
        return x

    @classmethod
    def from_file(cls, path, ids_file=None, metric="cosine", **kw):
        ids, x, differing = load_embeddings(path, ids_file)
        index = cls(x, ids, metric, **kw)
        index.differing = differing
        return index

    def _fp32(self, x):
        x = x.detach().to("cpu", F32)
        return torch.nn.functional.normalize(x, dim=1, eps=1e-12) if self.metric == "cosine" else x

    def _prepare(self, x, chunk=65536, normalize=None):
        normalize = self.metric == "cosine" if normalize is None else normalize
        out = torch.empty(x.shape[0], row_pitch(self.D), device=self.device, dtype=BF16)
        for lo in range(0, x.shape[0], chunk):
            out[lo:lo + chunk] = prepare_rows(x[lo:lo + chunk].detach().to(self.device, F32), normalize)
        return out

    def _search_args(self, queries, k, batch_size, exclude_self, rescore):
        """the refusals of search(); -> (exclude_self, the prepared foreign query rows or None, their fp32 rows for rescore)"""
        if not 1 <= k <= TOPK_MAX_K:
            raise ValueError(f"k must lie in [1, {TOPK_MAX_K}], got {k}")
        if batch_size < 1:
            raise ValueError(f"batch_size must be positive, got {batch_size}")
        own = queries is None
        if exclude_self is None:
            exclude_self = own
        if own:
            qrows, qf = None, self.fp32
        else:
            q = torch.as_tensor(queries)
            if q.dim() != 2 or q.shape[1] != self.D:
                raise ValueError(f"queries must be [B, {self.D}], got {tuple(q.shape)}")
            qrows, qf = self._prepare(q), (self._fp32(q) if rescore else None)
        if rescore and self.fp32 is None:
            raise ValueError("rescore needs the fp32 rows: build the index with keep_fp32=True")
        return exclude_self, qrows, qf

    def _workspace(self, nbytes):
        if self._ws is None or self._ws.numel() < nbytes:
            self._ws = torch.empty(max(nbytes, 1), device=self.device, dtype=torch.uint8)
        return self._ws

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


class ItemIndex(_Index):
    """A catalogue of N embeddings prepared for ia_sim_topk and held on the GPU.  ids: one label per row (default: the row number)."""

    def __init__(self, embeddings, ids=None, metric="cosine", keep_fp32=True, device=None):
        x = self._setup(embeddings, ids, metric, device)
        self.rows = self._prepare(x)                          # bf16 [N, pitch] on the GPU
        self.fp32 = self._fp32(x) if keep_fp32 else None      # fp32 (normalised) rows on the host, for rescore

    def search(self, queries=None, k=10, batch_size=4096, exclude_self=None, rescore=False):
        """(idx int64 [B, k], score fp32 [B, k]) on the CPU: for every query row the catalogue ROW NUMBERS of its k best rows (-1 / -inf
        in unused slots).  queries=None: every catalogue row queries the catalogue, and a row is kept out of its own list unless
        exclude_self=False.  With foreign queries exclude_self=True keeps catalogue row i from query i.  rescore: the scores of the
        returned rows recomputed as fp32 dots of the fp32 (normalised) rows and each list re-sorted by them (which rows are returned
        does not change)."""
        exclude_self, qrows, qf = self._search_args(queries, k, batch_size, exclude_self, rescore)
        if qrows is None:
            qrows = self.rows
        B = qrows.shape[0]
        idx = torch.empty(B, k, dtype=torch.int64)
        score = torch.empty(B, k, dtype=F32)
        for lo in range(0, B, batch_size):
            hi = min(B, lo + batch_size)
            skip = torch.arange(lo, hi, dtype=torch.int64, device=self.device) if exclude_self else None
            ws = self._workspace(_lib.load().ia_sim_topk_workspace_bytes(hi - lo, self.D, self.N, k, 0))
            i, s = sim_topk(qrows[lo:hi], self.rows, self.D, k, skip=skip, workspace=ws)
            idx[lo:hi], score[lo:hi] = i.cpu(), s.cpu()
        if rescore:
            idx, score = self._rescore(idx, score, qf)
        return idx, score


class IVFItemIndex(_Index):
    """The catalogue behind an inverted-file index.  nlist centroids (spherical k-means on a seeded sample of train_size rows, or the
    caller's `centroids`) partition the rows into lists, stored list by list; search() scans, for each query, only the nprobe lists
    whose centroids are most similar to it, so it is approximate: a neighbour in an unprobed list is missed.  With nprobe == nlist it
    returns what ItemIndex returns, bit for bit.

    Training clusters directions: the rows are normalised for it whatever the metric, and a query's probes are ranked by its inner
    product with the unit centroids, which orders them as its cosine does.  With metric="ip" a catalogue row of large norm in a list
    whose direction is far from the query's can have the largest inner product and still be missed.

    centroids / assignment: an explicit quantiser (fp32 [nlist, D], and the list of every row) instead of training -- how a saved
    index comes back (save / load).  Without `assignment` every row goes to the list of its most similar centroid, by the call that
    picks probes: a catalogue row used as a query probes its own list first.

    Layout: rows[list_off[l]:list_off[l + 1]] are the rows of list l in ascending original row; row_id[position] is the original
    row, inv its inverse."""

    def __init__(self, embeddings, ids=None, metric="cosine", nlist=None, nprobe=16, train_size=None, kmeans_iters=10, seed=0, keep_fp32=True,
                 device=None, centroids=None, assignment=None):
        x = self._setup(embeddings, ids, metric, device)
        N, D = self.N, self.D
        if N < 1:
            raise ValueError("IVFItemIndex: an empty catalogue has no lists")
        if nprobe < 1:
            raise ValueError(f"nprobe must be positive, got {nprobe}")
        self.nprobe, self.seed = int(nprobe), int(seed)
        if centroids is None:
            if assignment is not None:
                raise ValueError("assignment goes with the centroids it was made for: pass centroids too")
            nlist = max(1, min(N, round(4 * N ** 0.5))) if nlist is None else int(nlist)
            if not 1 <= nlist <= N:
                raise ValueError(f"nlist must lie in [1, {N}], got {nlist}")
            centroids = self._train(x, nlist, train_size, kmeans_iters)
        else:
            centroids = torch.as_tensor(centroids).detach().to(self.device, F32)
            if centroids.dim() != 2 or centroids.shape[1] != D or centroids.shape[0] < 1:
                raise ValueError(f"centroids must be [nlist, {D}], got {tuple(centroids.shape)}")
            if nlist is not None and nlist != centroids.shape[0]:
                raise ValueError(f"nlist {nlist} for {centroids.shape[0]} centroids")
        self.nlist = centroids.shape[0]
        self.centroids = centroids.cpu()                      # fp32 [nlist, D]
        self._cent = prepare_rows(centroids, False)           # the bf16 rows the probes are picked against
        rows = self._prepare(x)                               # original order, until the permutation below
        if assignment is None:
            assignment = torch.cat([sim_topk(rows[lo:lo + 262144], self._cent, D, 1)[0][:, 0] for lo in range(0, N, 262144)])
        else:
            assignment = torch.as_tensor(assignment).detach().to(self.device, torch.int64)
            if assignment.shape != (N,) or int(assignment.min()) < 0 or int(assignment.max()) >= self.nlist:
                raise ValueError(f"assignment must hold a list in [0, {self.nlist}) for each of the {N} rows")
        self.row_id = assignment.argsort(stable=True)         # position -> original row, ascending inside a list
        self.inv = torch.empty_like(self.row_id)
        self.inv[self.row_id] = torch.arange(N, device=self.device)
        self.rows = rows[self.row_id]                         # bf16 [N, pitch] on the GPU, list by list
        self._list_off = _offsets(torch.bincount(assignment, minlength=self.nlist))
        self.list_off, self.assignment = self._list_off.cpu(), assignment.cpu()
        self.fp32 = self._fp32(x) if keep_fp32 else None

    def _train(self, x, nlist, train_size, iters):
        N, D = self.N, self.D
        train_size = min(N, 256 * nlist) if train_size is None else int(train_size)
        if not nlist <= train_size <= N:
            raise ValueError(f"train_size must lie in [nlist, N] = [{nlist}, {N}], got {train_size}")
        g = torch.Generator().manual_seed(self.seed)
        sample = torch.randperm(N, generator=g)[:train_size]
        start = torch.randperm(train_size, generator=g)[:nlist]
        xs = self._prepare(x[sample.to(x.device)], normalize=True)
        cent = xs[start.to(self.device), :D].to(F32)
        for _ in range(iters):
            assign = sim_topk(xs, prepare_rows(cent, False), D, 1)[0][:, 0]
            sums, counts = centroid_sums(xs, D, assign.argsort(stable=True), _offsets(torch.bincount(assign, minlength=nlist)))
            norm = sums.norm(dim=1, keepdim=True)
            cent = torch.where((counts[:, None] > 0) & (norm > 0), sums / norm.clamp_min(1e-12), cent)   # an empty list keeps its centroid
        return cent

    def search(self, queries=None, k=10, batch_size=4096, exclude_self=None, rescore=False, nprobe=None, return_probes=False):
        """As ItemIndex.search (original catalogue row numbers and scores on the CPU, the same refusals), over the nprobe (default: the
        constructor's; at most nlist) lists nearest to each query.  return_probes: also the probed lists, int64 [B, nprobe], nearest
        first."""
        exclude_self, qrows, qf = self._search_args(queries, k, batch_size, exclude_self, rescore)
        nprobe = self.nprobe if nprobe is None else int(nprobe)
        if nprobe < 1:
            raise ValueError(f"nprobe must be positive, got {nprobe}")
        nprobe = min(nprobe, self.nlist)
        lib, dev, D = _lib.load(), self.device, self.D
        B = self.N if qrows is None else qrows.shape[0]
        idx = torch.empty(B, k, dtype=torch.int64)
        score = torch.empty(B, k, dtype=F32)
        probed = torch.empty(B, nprobe, dtype=torch.int64)
        for lo in range(0, B, batch_size):
            hi = min(B, lo + batch_size)
            qb = self.rows[self.inv[lo:hi]] if qrows is None else qrows[lo:hi]
            ws = self._workspace(max(lib.ia_sim_topk_workspace_bytes(hi - lo, D, self.nlist, nprobe, 0),
                                     lib.ia_sim_topk_groups_workspace_bytes((hi - lo) * nprobe, self.nlist, D, self.N, k, 0)))
            probes = sim_topk(qb, self._cent, D, nprobe, workspace=ws)[0]
            flat = probes.reshape(-1)
            order = flat.argsort(stable=True)                 # grouped row p holds the pair (query order[p] // nprobe, its list)
            rows_of = torch.empty_like(order)
            rows_of[order] = torch.arange(order.numel(), device=dev)
            src = torch.div(order, nprobe, rounding_mode="floor")
            skip = None
            if exclude_self:                                  # the position of catalogue row b; it lies in one list only
                own = torch.arange(lo, hi, device=dev)
                skip = torch.where(own < self.N, self.inv[own.clamp(max=self.N - 1)], torch.full_like(own, -1))[src]
            gi, gs = sim_topk_groups(qb[src], self.rows, _offsets(torch.bincount(flat, minlength=self.nlist)), self._list_off, D, k,
                                     label=self.row_id, skip=skip, workspace=ws, covered=True)
            i, s = sim_topk_fold(gi, gs, rows_of.view(hi - lo, nprobe))
            idx[lo:hi], score[lo:hi], probed[lo:hi] = i.cpu(), s.cpu(), probes.cpu()
        if rescore:
            idx, score = self._rescore(idx, score, qf)
        return (idx, score, probed) if return_probes else (idx, score)

    def list_sizes(self):
        """int64 [nlist] on the CPU"""
        return self.list_off[1:] - self.list_off[:-1]

    def summary(self):
        sizes = self.list_sizes()
        return (f"ivf nlist={self.nlist} empty={int((sizes == 0).sum())} list length min={int(sizes.min())} "
                f"median={int(sizes.median())} max={int(sizes.max())}")

    def save(self, path):
        torch.save({"centroids": self.centroids, "assignment": self.assignment, "N": self.N, "D": self.D, "metric": self.metric,
                    "nlist": self.nlist, "seed": self.seed}, path)

    @classmethod
    def load(cls, path, embeddings, ids=None, **kw):
        """The index save() wrote, over the same embeddings (they are not in the file)."""
        d = torch.load(path, map_location="cpu")
        x = torch.as_tensor(embeddings)
        metric = kw.pop("metric", d["metric"])
        for name, saved, given in (("N", d["N"], x.shape[0]), ("D", d["D"], x.shape[-1]), ("metric", d["metric"], metric)):
            if saved != given:
                raise ValueError(f"{path}: saved for {name} = {saved}, the embeddings have {name} = {given}")
        return cls(x, ids, metric, seed=d["seed"], centroids=d["centroids"], assignment=d["assignment"], **kw)


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
