"""Knowledge-graph pretraining of the PKGM / TransE embeddings (reference pkgm_pretrain.py over its vendored torchkge fork) on the
HIP engine: the models, the margin loss, the Bernoulli negative sampler, coupled-L2 Adam, the learning-rate schedule and the
trainer loop with the reference's quirks (INTEGRATION.md "PKGM knowledge-graph pretraining").

The tables (`ent_emb.weight`, `rel_emb.weight`) and the projection (`proj_mat.weight`) are fp32 and stay on the device; their
gradients are dense fp32 buffers that `ia_kgpt_score` accumulates into and `CoupledAdam.step` (ia_kgpt_adam_l2) clears.
"""
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


def load_ccks(data_dir):
    """train2id.txt (`from \\t rel \\t to`, integer ids as data_prepare.py writes them), entity2id.txt / relation2id.txt (`name \\t id`).
    The integer columns are used as ids (the reference maps them through the name-keyed dictionaries: INTEGRATION.md)."""
    rows = np.loadtxt(os.path.join(data_dir, "train2id.txt"), dtype=np.int64, delimiter="\t", ndmin=2)
    n_ent = _max_id(os.path.join(data_dir, "entity2id.txt")) + 1
    n_rel = _max_id(os.path.join(data_dir, "relation2id.txt")) + 1
    h, r, t = (torch.from_numpy(np.ascontiguousarray(rows[:, c])) for c in (0, 1, 2))
    for name, x, n in (("from", h, n_ent), ("to", t, n_ent), ("rel", r, n_rel)):
        if len(x) and (int(x.min()) < 0 or int(x.max()) >= n):
            raise ValueError(f"train2id.txt column '{name}' holds ids outside [0, {n}) of the id files")
    return KnowledgeGraph(h, t, r, n_ent, n_rel)


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
    def lr_lambda(current_step):
        if current_step < num_warmup_steps:
            return float(current_step) / float(max(1, num_warmup_steps))
        return max(0.0, float(num_training_steps - current_step) / float(max(1, num_training_steps - num_warmup_steps)))
    return lr_lambda


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
