"""Knowledge-graph pretraining of the PKGM / TransE embeddings (reference pkgm_pretrain.py over its vendored torchkge fork) on the
HIP engine: the models, the margin loss, the Bernoulli negative sampler, coupled-L2 Adam, the learning-rate schedule and the
trainer loop with the reference's quirks (INTEGRATION.md "PKGM knowledge-graph pretraining"); then what the trained tables are used
for: link-prediction ranks (LinkPredictionEvaluator, ia_kgpt_lp_rank) and completion (EntityInference / RelationInference,
ia_kgpt_topk).

The tables (`ent_emb.weight`, `rel_emb.weight`) and the projection (`proj_mat.weight`) are fp32 and stay on the device; their
gradients are dense fp32 buffers that `ia_kgpt_score` accumulates into and `CoupledAdam.step` (ia_kgpt_adam_l2) clears.
"""
import io
import math
import os

import numpy as np
import torch
from torch import nn

from .. import _lib
from .._lib import check, stream_ptr

F32 = torch.float32
KGPT_SCORE, KGPT_GRAD, KGPT_MARGIN = 0, 1, 2
NORMS = {"L1": 1, "L2": 2}


def _norm_code(dissimilarity_type):
    if dissimilarity_type not in NORMS:
        raise ValueError(f"dissimilarity_type {dissimilarity_type!r} is not supported: use 'L1' or 'L2' (the torus dissimilarities of "
                         "torchkge are not built)")
    return NORMS[dissimilarity_type]


class _KGScoreFn(torch.autograd.Function):
    """(h, t, r, nh, nt) -> (pos, neg) of TranslationModel.forward; the backward accumulates into the tables' .grad buffers."""

    @staticmethod
    def forward(ctx, anchor, model, h, t, r, nh, nt):
        pos, neg = model._run(h, t, r, nh, nt, KGPT_SCORE)
        ctx.model, ctx.saved = model, (h, t, r, nh, nt)
        return pos, neg

    @staticmethod
    def backward(ctx, dpos, dneg):
        z = torch.zeros(ctx.saved[0].shape[0], device=ctx.saved[0].device, dtype=F32)
        dpos = z if dpos is None else dpos.float().contiguous()
        dneg = z if dneg is None else dneg.float().contiguous()
        ctx.model._run(*ctx.saved, KGPT_GRAD, dpos=dpos, dneg=dneg)
        return (None,) * 7


class TranslationPretrainModel(nn.Module):
    """Common part of PKGMPretrainModel / TransEPretrainModel (torchkge models/interfaces.py TranslationModel + translation.py)."""
    use_proj = False

    def __init__(self, emb_dim, n_entities, n_relations, dissimilarity_type="L2"):
        super().__init__()
        self.norm = _norm_code(dissimilarity_type)
        self.dissimilarity_type = dissimilarity_type
        self.emb_dim, self.n_ent, self.n_rel = emb_dim, n_entities, n_relations
        if emb_dim % 4:
            raise ValueError(f"emb_dim must be a multiple of 4 (the kernels move 16-byte rows), got {emb_dim}")
        # init_embedding / init_linear_projection: Xavier-uniform, in the reference's construction order
        self.ent_emb = nn.Embedding(n_entities, emb_dim)
        nn.init.xavier_uniform_(self.ent_emb.weight.data)
        self.rel_emb = nn.Embedding(n_relations, emb_dim)
        nn.init.xavier_uniform_(self.rel_emb.weight.data)
        if self.use_proj:
            self.proj_mat = nn.Linear(emb_dim, emb_dim, bias=False)
            nn.init.xavier_uniform_(self.proj_mat.weight.data)
        # normalize_parameters() + the relation rows, at construction (host side: the model may not be on the device yet)
        self.ent_emb.weight.data = nn.functional.normalize(self.ent_emb.weight.data, p=2, dim=1)
        self.rel_emb.weight.data = nn.functional.normalize(self.rel_emb.weight.data, p=2, dim=1)
        self._anchor = torch.zeros((), requires_grad=True)
        self._ws = None

    def tables(self):
        return [self.ent_emb.weight, self.rel_emb.weight] + ([self.proj_mat.weight] if self.use_proj else [])

    def _ensure_grads(self):
        for p in self.tables():
            if p.grad is None or p.grad.shape != p.shape or p.grad.device != p.device:
                p.grad = torch.zeros_like(p)

    def _run(self, h, t, r, nh, nt, mode, dpos=None, dneg=None, margin=0.0):
        lib = _lib.load()
        ent = self.ent_emb.weight
        if not ent.is_cuda:
            raise RuntimeError("the knowledge-graph pretraining kernels run on the GPU: move the model with .cuda() first")
        idx = [x.contiguous().long() for x in (h, t, r, nh, nt)]
        B = idx[0].shape[0]
        if any(x.shape != (B,) or x.device != ent.device for x in idx):
            raise ValueError("h, t, r, nh, nt must be 1-D int64 tensors of one length on the model's device (one negative per fact)")
        D = self.emb_dim
        dev = ent.device
        pos = torch.empty(B, device=dev, dtype=F32)
        neg = torch.empty(B, device=dev, dtype=F32)
        loss = torch.empty(1, device=dev, dtype=F32) if mode == KGPT_MARGIN else None
        nbytes = lib.ia_kgpt_workspace_bytes(B, D, int(self.use_proj))
        if self._ws is None or self._ws.numel() < nbytes or self._ws.device != dev:
            self._ws = torch.empty(nbytes, device=dev, dtype=torch.uint8)
        proj = self.proj_mat.weight.data_ptr() if self.use_proj else None
        orders, grads = (None, None), (None, None, None)
        if mode != KGPT_SCORE:
            self._ensure_grads()
            h_, t_, r_, nh_, nt_ = idx
            orders = tuple(torch.argsort(k, stable=True).to(torch.int32) for k in (torch.cat([h_, nh_, t_, nt_]), torch.cat([r_, r_])))
            grads = (ent.grad.data_ptr(), self.rel_emb.weight.grad.data_ptr(), self.proj_mat.weight.grad.data_ptr() if self.use_proj else None)
        check(lib.ia_kgpt_score(ent.data_ptr(), self.rel_emb.weight.data_ptr(), proj, *(x.data_ptr() for x in idx), B, D, self.n_ent, self.n_rel,
                                self.norm, mode, float(margin), None if dpos is None else dpos.data_ptr(),
                                None if dneg is None else dneg.data_ptr(), pos.data_ptr(), neg.data_ptr(),
                                None if loss is None else loss.data_ptr(), *(None if o is None else o.data_ptr() for o in orders), *grads,
                                self._ws.data_ptr(), nbytes, stream_ptr()), "ia_kgpt_score")
        return (pos, neg, loss) if mode == KGPT_MARGIN else (pos, neg)

    def check_ids(self, h, t, r, nh, nt):
        """Raise if an id lies outside its table (the kernels would treat it as a zero row without a gradient)."""
        for name, x, n in (("h", h, self.n_ent), ("t", t, self.n_ent), ("nh", nh, self.n_ent), ("nt", nt, self.n_ent), ("r", r, self.n_rel)):
            if x.numel() and (int(x.min()) < 0 or int(x.max()) >= n):
                raise IndexError(f"{name} holds ids outside [0, {n})")

    def forward(self, heads, tails, relations, negative_heads, negative_tails):
        """(pos, neg) scores of the B facts and their B negatives (TranslationModel.forward with one negative per fact)."""
        self.check_ids(heads, tails, relations, negative_heads, negative_tails)
        return _KGScoreFn.apply(self._anchor, self, heads, tails, relations, negative_heads, negative_tails)

    def margin_step(self, h, t, r, nh, nt, margin):
        """Fused forward + MarginLoss + backward in one ia_kgpt_score call: returns (loss [1], pos, neg); the gradients accumulate into
        the tables' .grad.  Ids are not range-checked here (the trainer checks the KG once)."""
        pos, neg, loss = self._run(h, t, r, nh, nt, KGPT_MARGIN, margin=margin)
        return loss, pos, neg

    def normalize_parameters(self):
        """L2-normalise every entity row (torchkge normalize_parameters, called after every epoch)."""
        w = self.ent_emb.weight.data
        if w.is_cuda:
            check(_lib.load().ia_kgpt_row_normalize(w.data_ptr(), w.shape[0], w.shape[1], stream_ptr()), "ia_kgpt_row_normalize")
        else:
            self.ent_emb.weight.data = nn.functional.normalize(w, p=2, dim=1)

    def get_embeddings(self):
        self.normalize_parameters()
        return self.ent_emb.weight.data, self.rel_emb.weight.data


class PKGMPretrainModel(TranslationPretrainModel):
    """torchkge PKGMModel: score = -d(h + r, t) - d(h P^T, r), h / t L2-normalised, r not."""
    use_proj = True


class TransEPretrainModel(TranslationPretrainModel):
    """torchkge TransEModel: score = -d(h + r, t)."""
    use_proj = False


class MarginLoss(nn.Module):
    """torchkge MarginLoss: MarginRankingLoss(margin, reduction='sum') with target 1 = sum max(0, margin - pos + neg).  The trainer does
    not go through this module: its loss and gradients come out of the fused ia_kgpt_score call (TranslationPretrainModel.margin_step);
    this is the loss of the autograd path, over the [B] score vectors."""

    def __init__(self, margin):
        super().__init__()
        self.margin = margin

    def forward(self, positive_triplets, negative_triplets):
        return nn.functional.margin_ranking_loss(positive_triplets, negative_triplets, torch.ones_like(positive_triplets), margin=self.margin,
                                                 reduction="sum")


class CoupledAdam(torch.optim.Optimizer):
    """torch.optim.Adam (L2 weight decay added to the gradient, not AdamW's decoupled decay) over the dense fp32 tables, one
    ia_kgpt_adam_l2 launch per tensor; the launch also clears the gradient, so the next step's accumulation starts from zero."""

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0):
        super().__init__(params, dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay))
        self._clean = False

    @torch.no_grad()
    def step(self, closure=None):
        lib = _lib.load()
        for group in self.param_groups:
            b1, b2 = group["betas"]
            for p in group["params"]:
                if p.grad is None:
                    continue
                st = self.state[p]
                if not st:
                    st["step"] = 0
                    st["exp_avg"] = torch.zeros_like(p)
                    st["exp_avg_sq"] = torch.zeros_like(p)
                st["step"] += 1
                check(lib.ia_kgpt_adam_l2(p.data_ptr(), p.grad.data_ptr(), st["exp_avg"].data_ptr(), st["exp_avg_sq"].data_ptr(), p.numel(),
                                          group["lr"], b1, b2, group["eps"], group["weight_decay"], st["step"], stream_ptr()), "ia_kgpt_adam_l2")
        self._clean = True

    def zero_grad(self, set_to_none=False):
        """The step already left every gradient at zero; after a batch that did not step (gradient accumulation) they are cleared here."""
        if not self._clean:
            for group in self.param_groups:
                for p in group["params"]:
                    if p.grad is not None:
                        p.grad.zero_()
        self._clean = False


# ------------------------------------------------------------------------------------------------ data, sampler, schedule
class KnowledgeGraph:
    """The training graph of load_ccks: int64 heads / tails / relations in file order, n_ent / n_rel = max id + 1 of the id files."""

    def __init__(self, head_idx, tail_idx, relations, n_ent, n_rel):
        self.head_idx, self.tail_idx, self.relations = head_idx, tail_idx, relations
        self.n_ent, self.n_rel = n_ent, n_rel
        self.n_facts = len(head_idx)

    def __len__(self):
        return self.n_facts


def _max_id(path):
    m = -1
    with open(path, "r", encoding="utf-8") as f:
        for line in f:
            if line.strip():
                m = max(m, int(line.rstrip("\n").split("\t")[1]))
    return m


def _load_facts(data_dir, fname, n_ent, n_rel):
    """One `from \\t rel \\t to` id file as a KnowledgeGraph; ids outside the id files are a ValueError."""
    path = os.path.join(data_dir, fname)
    with open(path, "r", encoding="utf-8") as f:
        text = f.read()
    rows = np.loadtxt(io.StringIO(text), dtype=np.int64, delimiter="\t", ndmin=2) if text.strip() else np.zeros((0, 3), np.int64)
    h, r, t = (torch.from_numpy(np.ascontiguousarray(rows[:, c])) for c in (0, 1, 2))
    for name, x, n in (("from", h, n_ent), ("to", t, n_ent), ("rel", r, n_rel)):
        if len(x) and (int(x.min()) < 0 or int(x.max()) >= n):
            raise ValueError(f"{fname} column '{name}' holds ids outside [0, {n}) of the id files")
    return KnowledgeGraph(h, t, r, n_ent, n_rel)


def load_ccks(data_dir):
    """train2id.txt (`from \\t rel \\t to`, integer ids as data_prepare.py writes them), entity2id.txt / relation2id.txt (`name \\t id`).
    The integer columns are used as ids (the reference maps them through the name-keyed dictionaries: INTEGRATION.md)."""
    n_ent = _max_id(os.path.join(data_dir, "entity2id.txt")) + 1
    n_rel = _max_id(os.path.join(data_dir, "relation2id.txt")) + 1
    return _load_facts(data_dir, "train2id.txt", n_ent, n_rel)


class FilterGroups:
    """The filter of one side as CSR groups: for every (anchor, relation) key of the loaded facts the sorted, unique ids of the entities
    that complete a known fact -- torchkge's dict_of_tails[(h, r)] (anchor h, members t) or dict_of_heads[(t, r)] (anchor t, members h).
    `keys` = anchor * n_rel + relation, ascending; group g holds ids[offsets[g]:offsets[g + 1]].  Memory is O(loaded facts)."""

    def __init__(self, keys, offsets, ids, n_rel):
        self.keys, self.offsets, self.ids, self.n_rel = keys, offsets, ids, n_rel

    @classmethod
    def build(cls, anchor, relation, member, n_rel):
        anchor, relation, member = (np.asarray(x, dtype=np.int64) for x in (anchor, relation, member))
        key = anchor * n_rel + relation
        order = np.lexsort((member, key))
        key, member = key[order], member[order]
        keep = np.ones(len(key), dtype=bool)
        keep[1:] = (key[1:] != key[:-1]) | (member[1:] != member[:-1])
        key, member = key[keep], member[keep]
        keys, starts = np.unique(key, return_index=True)
        return cls(keys, np.append(starts, len(key)).astype(np.int64), member, n_rel)

    def __len__(self):
        return len(self.keys)

    def group_of(self, anchor, relation):
        """Group index of each (anchor, relation) pair, -1 where the key has no group."""
        key = np.asarray(anchor, dtype=np.int64) * self.n_rel + np.asarray(relation, dtype=np.int64)
        if not len(self.keys):
            return np.full(key.shape, -1, dtype=np.int64)
        g = np.minimum(np.searchsorted(self.keys, key), len(self.keys) - 1)
        return np.where(self.keys[g] == key, g, -1).astype(np.int64)

    def members(self, g):
        return self.ids[self.offsets[g]:self.offsets[g + 1]]


class KGFilters:
    """Both filters of link prediction over every loaded fact: `tails` keyed by (h, r), `heads` keyed by (t, r)."""

    def __init__(self, heads, tails):
        self.heads, self.tails = heads, tails

    @classmethod
    def build(cls, kgs):
        kgs = [k for k in kgs if k is not None]
        h, t, r = (np.concatenate([getattr(k, a).numpy() for k in kgs]) for a in ("head_idx", "tail_idx", "relations"))
        n_rel = kgs[0].n_rel
        return cls(FilterGroups.build(t, r, h, n_rel), FilterGroups.build(h, r, t, n_rel))


def load_ccks_splits(data_dir, do_eval, do_test):
    """The reference's load_ccks(data_dir, do_eval, do_test): train2id.txt, then valid2id.txt (do_eval) and test2id.txt (do_test), ids as
    written.  Returns (train, valid or None, test or None, KGFilters over all loaded facts).  Loading valid2id.txt widens the filter,
    so the test metrics depend on --do_eval, as in the reference."""
    n_ent = _max_id(os.path.join(data_dir, "entity2id.txt")) + 1
    n_rel = _max_id(os.path.join(data_dir, "relation2id.txt")) + 1
    train = _load_facts(data_dir, "train2id.txt", n_ent, n_rel)
    valid = _load_facts(data_dir, "valid2id.txt", n_ent, n_rel) if do_eval else None
    test = _load_facts(data_dir, "test2id.txt", n_ent, n_rel) if do_test else None
    return train, valid, test, KGFilters.build([train, valid, test])


def bernoulli_probs(kg):
    """BernoulliNegativeSampler.bern_probs (torchkge utils/operations.py get_bernoulli_probs): per relation tph / (tph + hpt), tph the
    mean number of facts per (head, relation), hpt per (relation, tail), in float64 then fp32; 0.5 for a relation without facts."""
    h, t, r = (x.numpy() for x in (kg.head_idx, kg.tail_idx, kg.relations))
    out = np.full(kg.n_rel, 0.5, dtype=np.float64)
    for rel in np.unique(r):
        sel = r == rel
        n = float(sel.sum())
        tph = n / len(np.unique(h[sel]))
        hpt = n / len(np.unique(t[sel]))
        out[rel] = tph / (tph + hpt)
    return torch.from_numpy(out.astype(np.float32))


def corrupt(h, t, r, bern_probs, n_ent, seed):
    """One negative per fact on the device (corrupt_kg -> corrupt_batch(n_neg=1)): (nh, nt)."""
    nh, nt = torch.empty_like(h), torch.empty_like(t)
    check(_lib.load().ia_kgpt_corrupt(h.data_ptr(), t.data_ptr(), r.data_ptr(), h.numel(), bern_probs.data_ptr(), bern_probs.numel(), n_ent,
                                      seed & (2 ** 64 - 1), nh.data_ptr(), nt.data_ptr(), stream_ptr()), "ia_kgpt_corrupt")
    return nh, nt


def n_batches(n, batch_size):
    return n // batch_size + (1 if n % batch_size else 0)


def schedule_steps(n_facts, batch_size, grad_accum, n_epochs, start_epoch, warmup_proportion):
    """(total, warm-up) optimizer steps of pkgm_pretrain.py: int(n / bs / gas) * (epochs - start_epoch), int(total * warmup)."""
    total = int(n_facts / batch_size / grad_accum) * (n_epochs - start_epoch)
    return total, int(total * warmup_proportion)


def linear_schedule_lambda(num_warmup_steps, num_training_steps):
    from ..train import linear_schedule_with_warmup
    return lambda current_step: linear_schedule_with_warmup(current_step, num_warmup_steps, num_training_steps)


def stepping_batches(n_batches_per_epoch, grad_accum):
    """Batches after which the optimizer steps.  The reference clears the gradients before EVERY batch, so a step sees only the
    gradient of the batch just before it (the others are computed and dropped)."""
    return [i for i in range(n_batches_per_epoch) if (i + 1) % grad_accum == 0]


def save_state_dict(model, path):
    torch.save({k: v.detach().cpu().clone() for k, v in model.state_dict().items()}, path)


def train(model, kg, optimizer, scheduler, *, n_epochs, batch_size, margin, save_path, start_epoch=0, save_epochs=None, log_steps=None,
          grad_accum=1, seed=0, logger=None):
    """utils/training.py Trainer.run on the device; returns the mean loss of every epoch."""
    import time
    dev = model.ent_emb.weight.device
    h, t, r = (x.to(dev) for x in (kg.head_idx, kg.tail_idx, kg.relations))
    probs = bernoulli_probs(kg).to(dev)
    nb = n_batches(len(kg), batch_size)
    means = []
    epoch = start_epoch - 1
    for epoch in range(start_epoch, n_epochs):
        t0 = time.perf_counter()
        nh, nt = corrupt(h, t, r, probs, kg.n_ent, seed * 1000003 + epoch)     # drawn once per epoch over the whole KG
        losses = []
        for i in range(nb):
            sl = slice(i * batch_size, (i + 1) * batch_size)
            optimizer.zero_grad()
            loss, _, _ = model.margin_step(h[sl], t[sl], r[sl], nh[sl], nt[sl], margin)
            if (i + 1) % grad_accum == 0:
                optimizer.step()
                scheduler.step()
            losses.append(loss)
            if log_steps is not None and i % log_steps == 0 and logger is not None:
                logger.info(f"[Epoch-{epoch + 1}] step: {i}, loss: {loss.item()}")
        mean = torch.cat(losses).sum().item() / nb
        model.normalize_parameters()
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        means.append(mean)
        if logger is not None:
            logger.info(f"Epoch {epoch + 1} | mean loss: {mean:.5f} | {len(kg) / dt:.0f} triples/s")
        if save_epochs is not None and (epoch + 1) % save_epochs == 0:
            save_state_dict(model, save_path.format(epoch + 1))
    save_state_dict(model, save_path.format(epoch + 1))
    return means


# ------------------------------------------------------------------------------------------------ link-prediction evaluation
LP_TAIL, LP_HEAD = 0, 1


class _DeviceGroups:
    """FilterGroups on the device (int64 offsets / ids) for ia_kgpt_lp_rank."""

    def __init__(self, groups, dev):
        self.groups = groups
        self.off = torch.from_numpy(groups.offsets).to(dev)
        ids = groups.ids if len(groups.ids) else np.zeros(1, np.int64)
        self.ids = torch.from_numpy(np.ascontiguousarray(ids)).to(dev)
        self.n = len(groups)


def _check_tables(ent, rel):
    """The tables the ranking and completion kernels read: contiguous 2-D fp32 of one width on one GPU.  Returns the device."""
    if not ent.is_cuda:
        raise RuntimeError("link-prediction ranking runs on the GPU")
    dev = ent.device
    for name, x in (("ent", ent), ("rel", rel)):
        if x.dtype != F32 or x.dim() != 2 or not x.is_contiguous() or x.device != dev:
            raise ValueError(f"{name} must be a contiguous 2-D fp32 table on {dev}, got {tuple(x.shape)} {x.dtype} on {x.device} "
                             f"(contiguous: {x.is_contiguous()})")
    if rel.shape[1] != ent.shape[1]:
        raise ValueError(f"ent and rel widths differ: {ent.shape[1]} != {rel.shape[1]}")
    return dev


def lp_rank(ent, rel, h, t, r, norm, side, groups=None, q_grp=None, want_scores=False, workspace=None):
    """One ia_kgpt_lp_rank call over B queries on one side (LP_TAIL: rank t among all entities, LP_HEAD: rank h), on the raw tables.
    groups: a FilterGroups (or its _DeviceGroups) and q_grp the group index of each query (int64 [B], -1 = none); None = unfiltered.
    Returns (rank, filt_rank) int64 [B], and the fp32 [B, n_ent] scores the ranks compare when want_scores."""
    lib = _lib.load()
    dev = _check_tables(ent, rel)
    h, t, r = (x.to(dev).contiguous().long() for x in (h, t, r))
    B = h.shape[0]
    n_ent, D = ent.shape
    rank = torch.empty(B, device=dev, dtype=torch.int64)
    filt = torch.empty(B, device=dev, dtype=torch.int64)
    scores = torch.empty(B, n_ent, device=dev, dtype=F32) if want_scores else None
    nbytes = lib.ia_kgpt_lp_workspace_bytes(B, D)
    if workspace is None or workspace.numel() < nbytes:
        workspace = torch.empty(nbytes, device=dev, dtype=torch.uint8)
    gp = (None, None, 0, None)
    if groups is not None:
        dg = groups if isinstance(groups, _DeviceGroups) else _DeviceGroups(groups, dev)
        qg = torch.as_tensor(q_grp, dtype=torch.int64).to(dev).contiguous()
        gp = (dg.off.data_ptr(), dg.ids.data_ptr(), dg.n, qg.data_ptr())
    check(lib.ia_kgpt_lp_rank(ent.data_ptr(), rel.data_ptr(), h.data_ptr(), t.data_ptr(), r.data_ptr(), B, D, n_ent, rel.shape[0], norm, side,
                              *gp, rank.data_ptr(), filt.data_ptr(), None if scores is None else scores.data_ptr(), workspace.data_ptr(),
                              nbytes, stream_ptr()), "ia_kgpt_lp_rank")
    return (rank, filt, scores) if want_scores else (rank, filt)


class NotYetEvaluatedError(RuntimeError):
    pass


class LinkPredictionEvaluator:
    """torchkge LinkPredictionEvaluator on the device: raw and filtered ranks of the true head and the true tail of every fact of `kg`
    among all entities, scored on the model's raw tables (no normalisation, no projection term: PKGM ranks like TransE).  `filters`
    (KGFilters) hold the known facts of every loaded split.  The metrics are torchkge's fp32 expressions over the CPU int64 ranks."""

    def __init__(self, model, knowledge_graph, filters):
        self.model, self.kg, self.filters = model, knowledge_graph, filters
        n = knowledge_graph.n_facts
        self.rank_true_heads = torch.empty(n, dtype=torch.int64)
        self.rank_true_tails = torch.empty(n, dtype=torch.int64)
        self.filt_rank_true_heads = torch.empty(n, dtype=torch.int64)
        self.filt_rank_true_tails = torch.empty(n, dtype=torch.int64)
        self.evaluated = False

    @torch.no_grad()
    def evaluate(self, b_size, verbose=False):
        """Ranks in file order, b_size queries per kernel call (the ranks do not depend on it).  verbose is accepted for torchkge's
        signature; there is no progress bar."""
        if b_size <= 0:
            raise ValueError(f"b_size must be positive, got {b_size}")
        ent, rel = self.model.ent_emb.weight.data, self.model.rel_emb.weight.data
        dev = ent.device
        kg = self.kg
        n = kg.n_facts
        h, t, r = (x.to(dev) for x in (kg.head_idx, kg.tail_idx, kg.relations))
        hn, tn, rn = (x.numpy() for x in (kg.head_idx, kg.tail_idx, kg.relations))
        sides = ((LP_TAIL, _DeviceGroups(self.filters.tails, dev), self.filters.tails.group_of(hn, rn)),
                 (LP_HEAD, _DeviceGroups(self.filters.heads, dev), self.filters.heads.group_of(tn, rn)))
        out = {s: (torch.empty(n, device=dev, dtype=torch.int64), torch.empty(n, device=dev, dtype=torch.int64)) for s, _, _ in sides}
        ws = torch.empty(_lib.load().ia_kgpt_lp_workspace_bytes(max(1, min(b_size, n)), ent.shape[1]), device=dev, dtype=torch.uint8)
        for i0 in range(0, n, b_size):
            sl = slice(i0, min(n, i0 + b_size))
            for side, dg, qg in sides:
                rk, fr = lp_rank(ent, rel, h[sl], t[sl], r[sl], self.model.norm, side, dg, qg[sl], workspace=ws)
                out[side][0][sl] = rk
                out[side][1][sl] = fr
        self.rank_true_tails, self.filt_rank_true_tails = (x.cpu() for x in out[LP_TAIL])
        self.rank_true_heads, self.filt_rank_true_heads = (x.cpu() for x in out[LP_HEAD])
        self.evaluated = True

    def _check(self):
        if not self.evaluated:
            raise NotYetEvaluatedError("Evaluator not evaluated call LinkPredictionEvaluator.evaluate")

    def mean_rank(self):
        self._check()
        sum_ = (self.rank_true_heads.float().mean() + self.rank_true_tails.float().mean()).item()
        filt_sum = (self.filt_rank_true_heads.float().mean() + self.filt_rank_true_tails.float().mean()).item()
        return sum_ / 2, filt_sum / 2

    def hit_at_k_heads(self, k=10):
        self._check()
        head_hit = (self.rank_true_heads <= k).float().mean()
        filt_head_hit = (self.filt_rank_true_heads <= k).float().mean()
        return head_hit.item(), filt_head_hit.item()

    def hit_at_k_tails(self, k=10):
        self._check()
        tail_hit = (self.rank_true_tails <= k).float().mean()
        filt_tail_hit = (self.filt_rank_true_tails <= k).float().mean()
        return tail_hit.item(), filt_tail_hit.item()

    def hit_at_k(self, k=10):
        self._check()
        head_hit, filt_head_hit = self.hit_at_k_heads(k=k)
        tail_hit, filt_tail_hit = self.hit_at_k_tails(k=k)
        return (head_hit + tail_hit) / 2, (filt_head_hit + filt_tail_hit) / 2

    def mrr(self):
        self._check()
        head_mrr = (self.rank_true_heads.float() ** (-1)).mean()
        tail_mrr = (self.rank_true_tails.float() ** (-1)).mean()
        filt_head_mrr = (self.filt_rank_true_heads.float() ** (-1)).mean()
        filt_tail_mrr = (self.filt_rank_true_tails.float() ** (-1)).mean()
        return (head_mrr + tail_mrr).item() / 2, (filt_head_mrr + filt_tail_mrr).item() / 2

    def results_text(self, k=None, n_digits=3):
        """The lines print_results prints, as one string."""
        self._check()
        if k is None:
            k = 10
        lines = []
        for i in ([k] if isinstance(k, int) else list(k)):
            lines.append("Hit@{} : {} \t\t Filt. Hit@{} : {}".format(i, round(self.hit_at_k(k=i)[0], n_digits), i,
                                                                     round(self.hit_at_k(k=i)[1], n_digits)))
        lines.append("Mean Rank : {} \t Filt. Mean Rank : {}".format(int(self.mean_rank()[0]), int(self.mean_rank()[1])))
        lines.append("MRR : {} \t\t Filt. MRR : {}".format(round(self.mrr()[0], n_digits), round(self.mrr()[1], n_digits)))
        return "\n".join(lines) + "\n"

    def print_results(self, k=None, n_digits=3):
        print(self.results_text(k, n_digits), end="", flush=True)


# ------------------------------------------------------------------------------------------------ completion (torchkge inference.py)
TOPK_TAILS, TOPK_HEADS, TOPK_RELS = 0, 1, 2
TOPK_MAX_K = 64


class WrongArgumentsError(ValueError):
    """torchkge.exceptions.WrongArgumentsError."""


def relation_filter_groups(kgs):
    """The filter of relation completion over every fact of `kgs`: FilterGroups keyed by (head, tail) whose members are the known
    relations -- torchkge's dict_of_rels[(h, t)].  The key base is n_ent (key = head * n_ent + tail)."""
    kgs = [k for k in kgs if k is not None]
    h, t, r = (np.concatenate([getattr(k, a).numpy() for k in kgs]) for a in ("head_idx", "tail_idx", "relations"))
    return FilterGroups.build(h, t, r, kgs[0].n_ent)


def filter_groups_from_dict(dictionary, key_base):
    """A torchkge filter dictionary {(key1, key2): iterable of ids} (dict_of_tails, dict_of_heads, dict_of_rels) as FilterGroups with
    keys key1 * key_base + key2: key_base = n_rel for the entity dictionaries, n_ent for the relation dictionary."""
    a, b, m = [], [], []
    for (k1, k2), ids in dictionary.items():
        ids = [int(i) for i in ids]
        a += [int(k1)] * len(ids)
        b += [int(k2)] * len(ids)
        m += ids
    return FilterGroups.build(np.asarray(a, np.int64), np.asarray(b, np.int64), np.asarray(m, np.int64), key_base)


def kg_topk(ent, rel, a, b, norm, mode, k, groups=None, q_grp=None, max_splits=0, workspace=None):
    """One ia_kgpt_topk call: the k best candidates of B queries on the raw tables.  TOPK_TAILS: a = heads, b = relations;
    TOPK_HEADS: a = tails, b = relations; TOPK_RELS: a = heads, b = tails (candidates = relation rows).  groups / q_grp as in lp_rank:
    the members of a query's group are never returned.  Returns (idx int64 [B, k], score fp32 [B, k]) on the device, best first in the
    order (score descending, id ascending); unused slots hold -1 / -inf."""
    lib = _lib.load()
    dev = _check_tables(ent, rel)
    a, b = (torch.as_tensor(x).to(dev).contiguous().long() for x in (a, b))
    B = a.shape[0]
    if a.shape != (B,) or b.shape != (B,):
        raise ValueError(f"a and b must be 1-D id tensors of one length, got {tuple(a.shape)} and {tuple(b.shape)}")
    if not 1 <= k <= TOPK_MAX_K:
        raise ValueError(f"k must lie in [1, {TOPK_MAX_K}], got {k}")
    n_ent, D = ent.shape
    n_cand = rel.shape[0] if mode == TOPK_RELS else n_ent
    idx = torch.empty(B, k, device=dev, dtype=torch.int64)
    score = torch.empty(B, k, device=dev, dtype=F32)
    if B == 0:
        return idx, score
    nbytes = lib.ia_kgpt_topk_workspace_bytes(B, D, n_cand, k, max_splits)
    if workspace is None or workspace.numel() < nbytes:
        workspace = torch.empty(max(nbytes, 1), device=dev, dtype=torch.uint8)
    gp = (None, None, 0, None)
    if groups is not None:
        dg = groups if isinstance(groups, _DeviceGroups) else _DeviceGroups(groups, dev)
        qg = torch.as_tensor(q_grp, dtype=torch.int64).to(dev).contiguous()
        gp = (dg.off.data_ptr(), dg.ids.data_ptr(), dg.n, qg.data_ptr())
    check(lib.ia_kgpt_topk(ent.data_ptr(), rel.data_ptr(), a.data_ptr(), b.data_ptr(), B, D, n_ent, rel.shape[0], norm, mode, *gp, k,
                           max_splits, idx.data_ptr(), score.data_ptr(), workspace.data_ptr(), workspace.numel(), stream_ptr()),
          "ia_kgpt_topk")
    return idx, score


class _Inference:
    """Common part of EntityInference / RelationInference: queries (a, b) in order, b_size per kernel call."""

    def _setup(self, model, a, b, top_k, mode, dictionary, key_base):
        self.model, self.top_k, self.dictionary = model, top_k, dictionary
        self._a, self._b, self._mode = torch.as_tensor(a).long().cpu(), torch.as_tensor(b).long().cpu(), mode
        if isinstance(dictionary, dict):
            dictionary = filter_groups_from_dict(dictionary, key_base)       # once, on the host
        self._groups = dictionary
        n = len(self._a)
        self.predictions = torch.empty(n, top_k, dtype=torch.int64)
        self.scores = torch.empty(n, top_k, dtype=F32)

    @torch.no_grad()
    def evaluate(self, b_size, verbose=True):
        """Fills .predictions (int64 [n, top_k]) and .scores (fp32 [n, top_k]) on the CPU; they do not depend on b_size.  verbose is
        accepted for torchkge's signature; there is no progress bar."""
        if b_size <= 0:
            raise ValueError(f"b_size must be positive, got {b_size}")
        ent, rel = self.model.ent_emb.weight.data, self.model.rel_emb.weight.data
        if not ent.is_cuda:
            raise RuntimeError("link-prediction ranking runs on the GPU")
        dev = ent.device
        n = len(self._a)
        a, b = self._a.to(dev), self._b.to(dev)
        dg = qg = None
        if self._groups is not None:
            dg = _DeviceGroups(self._groups, dev)
            qg = torch.from_numpy(self._groups.group_of(self._a.numpy(), self._b.numpy())).to(dev)
        pred = torch.empty(n, self.top_k, device=dev, dtype=torch.int64)
        sc = torch.empty(n, self.top_k, device=dev, dtype=F32)
        for i0 in range(0, n, b_size):
            sl = slice(i0, min(n, i0 + b_size))
            pred[sl], sc[sl] = kg_topk(ent, rel, a[sl], b[sl], self.model.norm, self._mode, self.top_k, dg, None if qg is None else qg[sl])
        self.predictions, self.scores = pred.cpu(), sc.cpu()


class EntityInference(_Inference):
    """torchkge EntityInference on the device: the top_k entities that complete (known entity, known relation), the known entity being
    the head (missing='tails') or the tail (missing='heads'), scored on the model's raw tables (PKGM infers like TransE).  dictionary:
    a FilterGroups or torchkge's dict_of_tails / dict_of_heads {(entity, relation): ids}; its members are never predicted."""

    def __init__(self, model, known_entities, known_relations, top_k=1, missing="tails", dictionary=None):
        if missing not in ("heads", "tails"):
            raise WrongArgumentsError("missing entity should either be 'heads' or 'tails'")
        self.missing = missing
        self.known_entities, self.known_relations = known_entities, known_relations
        self._setup(model, known_entities, known_relations, top_k, TOPK_TAILS if missing == "tails" else TOPK_HEADS, dictionary,
                    model.n_rel if isinstance(dictionary, dict) else None)


class RelationInference(_Inference):
    """torchkge RelationInference on the device: the top_k relations that complete (entities1 = heads, entities2 = tails).  dictionary:
    a FilterGroups (relation_filter_groups) or a dict {(head, tail): relation ids}."""

    def __init__(self, model, entities1, entities2, top_k=1, dictionary=None):
        self.entities1, self.entities2 = entities1, entities2
        self._setup(model, entities1, entities2, top_k, TOPK_RELS, dictionary, model.n_ent if isinstance(dictionary, dict) else None)
