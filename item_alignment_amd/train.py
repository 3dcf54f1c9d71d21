"""Train / eval / predict harness shared by finetune_{text,image,multimodal}.py; the other training scripts call its pieces.

It reproduces the reference's loop (finetune_multimodal.py:371-468 train, :470-563 eval, :565-569 checkpoint,
:661-775 predict; the same blocks in finetune_text.py:396-492 and finetune_image.py:310-348): zero_grad ->
forward -> loss (/ accumulation) -> backward -> AdamW(beta=(0.9,0.98)) + linear warm-up/decay schedule, loss
logged every log_steps, P/R/F1 swept over thresholds 0.1..0.9, state_dict saved per epoch under the reference's
file names.  What is new: the optimiser is one fused HIP launch over the parameter arena, `--fp16` selects the
engine's bf16 path (it is always on for the HIP models; there is no GradScaler), and the loop is data-parallel
when launched with torch.distributed.run (RANK / WORLD_SIZE / LOCAL_RANK): the global batch (--train_batch_size
keeps its meaning "total batch size") is sharded across ranks and gradients are all-reduced over RCCL.
"""
import json
import os
import random

import numpy as np
import torch
from torch.utils.data import DataLoader, Subset

from . import dist as iadist
from .utils import logger


def seed_everything(seed):
    random.seed(seed)
    np.random.seed(seed)
    torch.manual_seed(seed)
    if torch.cuda.is_available():
        torch.cuda.manual_seed_all(seed)


def linear_schedule_with_warmup(step, num_warmup_steps, num_training_steps):
    """transformers.get_linear_schedule_with_warmup lambda (reference finetune_multimodal.py:315); the two other names forward here"""
    if step < num_warmup_steps:
        return float(step) / float(max(1, num_warmup_steps))
    return max(0.0, float(num_training_steps - step) / float(max(1, num_training_steps - num_warmup_steps)))


class TorchAdamW:
    """Reference optimiser construction (two parameter groups, finetune_multimodal.py:296-308) for models that do not
    live in a HIP parameter arena (the TextCNN CPU plumbing config)."""

    def __init__(self, model, lr, eps, weight_decay):
        no_decay = ["bias", "LayerNorm.weight"]
        groups = [{"params": [p for n, p in model.named_parameters() if not any(nd in n for nd in no_decay)], "weight_decay": weight_decay},
                  {"params": [p for n, p in model.named_parameters() if any(nd in n for nd in no_decay)], "weight_decay": 0.0}]
        self.opt = torch.optim.AdamW(groups, lr=lr, eps=eps, betas=(0.9, 0.98))
        self.base_lr = lr

    def zero_grad(self):
        self.opt.zero_grad()

    def step(self, lr_mult, grad_scale=1.0):
        for g in self.opt.param_groups:
            g["lr"] = self.base_lr * lr_mult
        self.opt.step()


class ArenaAdamW:
    """Fused AdamW over the flat parameter arena (one HIP launch; same update rule and parameter-group semantics)."""

    def __init__(self, model, lr, eps, weight_decay, betas=(0.9, 0.98)):
        self.arena = model.param_arena
        self.base_lr, self.eps, self.wd, self.betas = lr, eps, weight_decay, betas

    def zero_grad(self):
        self.arena.zero_grad()

    def step(self, lr_mult, grad_scale=1.0):
        self.arena.adamw_step(self.base_lr * lr_mult, betas=self.betas, eps=self.eps, weight_decay=self.wd, grad_scale=grad_scale)


def clipped_adamw_step(arena, lr, max_grad_norm, inv_world=1.0, *, betas, eps, weight_decay):
    """clip_grad_norm_(model.parameters(), max_grad_norm) as a factor on the gradients inside the fused optimiser step.  inv_world:
    what GradBucketReducer.finish() returned -- the arena holds the SUM over the ranks, the norm is the average's, on every rank"""
    norm = arena.grad.norm().item() * inv_world
    scale = min(1.0, max_grad_norm / (norm + 1e-6)) * inv_world
    arena.adamw_step(lr, betas=betas, eps=eps, weight_decay=weight_decay, grad_scale=scale)


class ArenaLAMB:
    """LAMB over the flat parameter arena (arena.lamb_step): ArenaAdamW's interface, the script's own betas, epsilon and weight decay"""

    def __init__(self, model, lr, eps, weight_decay, betas=(0.9, 0.98)):
        self.arena = model.param_arena
        self.base_lr, self.eps, self.wd, self.betas = lr, eps, weight_decay, betas

    def zero_grad(self):
        self.arena.zero_grad()

    def step(self, lr_mult, grad_scale=1.0):
        self.arena.lamb_step(self.base_lr * lr_mult, betas=self.betas, eps=self.eps, weight_decay=self.wd, grad_scale=grad_scale)


def clipped_lamb_step(arena, lr, max_grad_norm, inv_world=1.0, *, betas, eps, weight_decay):
    """clipped_adamw_step's clipping with the LAMB update: the same factor, formed on the device from the gradient norm inside the
    optimiser step (no .item(), no host sync)"""
    arena.lamb_step(lr, betas=betas, eps=eps, weight_decay=weight_decay, grad_scale=inv_world, max_grad_norm=max_grad_norm)


OPTIMIZERS = ("adamw", "lamb")


def add_optimizer_flag(parser):
    parser.add_argument("--optimizer", default="adamw", choices=OPTIMIZERS,
                        help="adamw: the reference's optimiser.  lamb: the same direction rescaled per parameter tensor by |w| / |u| "
                             "(You et al. 2020), for large total batches; keeps this script's betas, epsilon, weight decay and schedule")


def require_arena_for_lamb(args, is_hip):
    if getattr(args, "optimizer", "adamw") == "lamb" and not is_hip:
        raise SystemExit("--optimizer lamb runs over the GPU parameter arena: this model has none here (TextCNN on the CPU); use --optimizer adamw")


def clipped_step(args):
    """the clipped optimiser step --optimizer selects"""
    return clipped_lamb_step if getattr(args, "optimizer", "adamw") == "lamb" else clipped_adamw_step


def accumulate_step(opt, loss, last, accumulation_steps, lr_mult, reducer=None, average_grads=None):
    """backward() of one micro-batch; on the `last` one of an optimiser step also the reduction over the ranks, opt.step(lr_mult)
    and zero_grad.  average_grads: called before the step where no reducer averages (plain torch models on several ranks).  -> last"""
    if accumulation_steps > 1:
        loss = loss / accumulation_steps
    if reducer is not None:       # collectives only start in the backward that completes the accumulated gradient
        reducer.armed = last
    loss.backward()
    if last:
        if average_grads is not None:
            average_grads()
        opt.step(lr_mult, grad_scale=reducer.finish() if reducer is not None else 1.0)
        opt.zero_grad()
    return last


def model_dir(args, kind_fields):
    """reference finetune_multimodal.py:349 / finetune_text.py:373 / finetune_image.py:287 directory naming."""
    return os.path.join(args.output_dir, "-".join(str(getattr(args, f)) for f in kind_fields))


def dump_hyperparameters(out_dir, args, config):
    with open(os.path.join(out_dir, "hyperparamter.txt"), "w") as f:
        f.write(f"{args}\n\n\n{config}\n")          # print(args), print("\n"), print(config)


def log_threshold_sweep(probs, labels, prefix):
    """P / R / F1 at the thresholds 0.1 .. 0.9, one log line each (reference finetune_multimodal.py:540-563)"""
    from sklearn.metrics import f1_score, precision_score, recall_score
    for threshold in np.arange(0.1, 1.0, 0.1):
        pred = probs >= threshold
        p, r, f1 = precision_score(labels, pred, zero_division=0), recall_score(labels, pred, zero_division=0), f1_score(labels, pred, zero_division=0)
        logger.info(f"{prefix}threshold={threshold}, precision={p}, recall={r}, f1={f1}")


def write_pair_embeddings(path, loader, rows_of, threshold, log_steps):
    """The deepAI_result_*.jsonl of --do_pred.  rows_of(batch), under no_grad -> (src ids, tgt ids, src embeddings, tgt embeddings),
    the embeddings as numpy rows, or None for a batch that lost all its rows"""
    text = lambda v: ",".join(str(x) for x in v) if isinstance(v, np.ndarray) else str(v)
    with open(path, "w", encoding="utf-8") as w, torch.no_grad():
        for step, batch in enumerate(loader):
            rows = rows_of(batch)
            if rows is None:
                continue
            for sid, tid, s, t in zip(*rows):
                w.write(json.dumps({"src_item_id": sid, "src_item_emb": f"[{text(s)}]", "tgt_item_id": tid, "tgt_item_emb": f"[{text(t)}]",
                                    "threshold": threshold}) + "\n")
            if log_steps is not None and step % log_steps == 0:
                logger.info(f"[Prediction] {step} samples processed")
    logger.info("[Prediction] Finished")


class BatchFeeder:
    """A collate output -> what the model is called with: --gpu_jpeg decode, the GPU image pipeline, the move to the device."""

    def __init__(self, args, device):
        self.size, self.device, self.pipelines = int(getattr(args, "image_size", 0) or 0), device, {}
        nw = int(getattr(args, "num_workers", 0) or 0)
        # never fork() a process that owns HIP streams: workers come from a clean fork server and only see the pickled dataset
        self.loader_kw = dict(num_workers=nw, pin_memory=(device.type == "cuda"), persistent_workers=False,
                              **({"multiprocessing_context": "forkserver"} if nw > 0 else {}))

    def pipeline(self):
        from .data.gpu_preproc import GpuImagePipeline
        pipe = self.pipelines.get(self.size)
        if pipe is None:
            pipe = self.pipelines[self.size] = GpuImagePipeline(self.size, self.device)
        return pipe

    def decode_jpeg(self, batch):
        """--gpu_jpeg: the JpegImage samples of every image element of a collate output are decoded in one batched call on the GPU
        (data/jpeg.py; one status read per batch) and become RawImage samples whose frame already lives on the device.  A pair one of
        whose images neither the GPU nor Pillow could decode is dropped from every element of the batch, ids included - the
        reference's rule for an image that fails to load (data.py:44, :84), applied one stage later.  None: no row is left."""
        from .data.datasets import RawImageBatch
        from .data.jpeg import JpegImage, drop_rows
        raws = [t for t in batch if isinstance(t, RawImageBatch)]
        if not any(isinstance(it, JpegImage) for t in raws for it in t.items):
            return batch
        flat = self.pipeline().decode([it for t in raws for it in t.items])
        n, decoded = len(raws[0]), {}
        for j, t in enumerate(raws):
            decoded[id(t)] = flat[j * n:(j + 1) * n]
        keep = [all(d[i] is not None for d in decoded.values()) for i in range(n)]
        batch = drop_rows(tuple(RawImageBatch(decoded[id(t)]) if isinstance(t, RawImageBatch) else t for t in batch), keep)
        return batch if any(keep) else None

    def to_device(self, batch):
        """tensors move; a RawImageBatch becomes normalised [B, 3, S, S] on the device (data/gpu_preproc.py: the reference's transform)"""
        from .data.datasets import RawImageBatch
        return tuple(self.pipeline().process(t.items) if isinstance(t, RawImageBatch)
                     else (t.to(device=self.device, non_blocking=True) if torch.is_tensor(t) else t) for t in batch)


def evaluate(args, model, dataset, collate_fn, call_model, feeder, ranks, tag):
    """Scores the whole set.  Under data parallelism every rank scores positions rank::world and the (score, label) rows of
    all ranks are concatenated everywhere: no rank sits in a collective while another one evaluates alone.  The
    P/R/F1 sweep does not depend on the order, and a rank may come back with fewer rows than it was dealt (the collates drop
    samples whose image failed to load, data.py:44,84) or with none at all."""
    model.eval()
    rank, world = ranks.rank, ranks.world
    mine = list(range(rank, len(dataset), world)) if world > 1 else None
    loader = DataLoader(dataset if mine is None else Subset(dataset, mine), batch_size=args.eval_batch_size, shuffle=False,
                        collate_fn=collate_fn, **feeder.loader_kw)
    probs_all, labels_all = None, None
    with torch.no_grad():
        for batch in loader:
            batch = feeder.decode_jpeg(batch)
            if batch is None:
                continue
            b = feeder.to_device(batch[2:])
            out = call_model(model, b)
            probs, labels = out.probs.float().cpu().numpy(), b[-1].cpu().numpy()
            if probs.ndim == 2:
                # RobertaTwoTower / PKGMTwoTower / RobertaImageTwoTower hand back softmax probs [B, 2] (quirk A3); the
                # reference appends them flat and its sklearn call then fails on 2B vs B samples: score P(match) instead
                probs = probs[:, 1]
            probs_all = probs if probs_all is None else np.append(probs_all, probs)
            labels_all = labels if labels_all is None else np.append(labels_all, labels)
    if world > 1:
        rows = np.empty((0, 2)) if probs_all is None else np.stack([np.asarray(probs_all, np.float64), np.asarray(labels_all, np.float64)], 1)
        rows = iadist.gather_rows(rows)
        probs_all, labels_all = rows[:, 0], rows[:, 1].astype(np.int64)
    if rank == 0 and probs_all is not None:
        log_threshold_sweep(probs_all, labels_all, f"[{tag}] ")


def predict(args, model, dataset, collate_fn, call_model, feeder, out_dir):
    """--do_pred (rank 0 alone): the classifier's last layer as weights.json, the pair embeddings of the test set as jsonl"""
    model.eval()
    head = model.classifier.out_proj
    json.dump({"w": head.weight.detach().cpu().numpy().tolist(), "b": head.bias.detach().cpu().numpy().tolist()},
              open(os.path.join(out_dir, "weights.json"), "w", encoding="utf-8"), ensure_ascii=False)
    loader = DataLoader(dataset, batch_size=args.eval_batch_size, shuffle=False, collate_fn=collate_fn, **feeder.loader_kw)

    def rows_of(batch):
        batch = feeder.decode_jpeg(batch)
        if batch is None:
            return None
        out = call_model(model, feeder.to_device(batch[2:]))
        return batch[0], batch[1], out.src_embeds.float().cpu().numpy(), out.tgt_embeds.float().cpu().numpy()

    write_pair_embeddings(os.path.join(out_dir, f"deepAI_result_{getattr(args, 'pred_tag', '')}threshold={args.threshold}.jsonl"), loader, rows_of,
                          args.threshold, args.log_steps)


def train_epochs(args, model, datasets, collate_fn, call_model, checkpoint_name, feeder, ranks, out_dir):
    from .models import functional as Fn
    rank, world, device = ranks.rank, ranks.world, feeder.device
    is_hip = hasattr(model, "param_arena") and device.type == "cuda"
    train_ds = datasets["train"]
    per_rank = args.train_batch_size // world
    if per_rank * world != args.train_batch_size:
        raise ValueError(f"--train_batch_size {args.train_batch_size} must be divisible by the world size {world}")
    require_arena_for_lamb(args, is_hip)
    opt_cls = ArenaLAMB if getattr(args, "optimizer", "adamw") == "lamb" else (ArenaAdamW if is_hip else TorchAdamW)
    opt = opt_cls(model, args.learning_rate, args.adam_epsilon, args.weight_decay)
    steps_per_epoch = int(len(train_ds) / args.train_batch_size / args.gradient_accumulation_steps)
    total = steps_per_epoch * (args.num_train_epochs - args.start_epoch)
    warm = int(total * args.warmup_proportion)
    reducer = ranks.attach(model.param_arena, always=True) if is_hip else None
    # plain torch models (TextCNN) under several ranks: average the gradients over the ranks before the step
    average_grads = (lambda: iadist.all_reduce_grads(model, world)) if reducer is None and world > 1 else None
    if rank == 0:
        dump_hyperparameters(out_dir, args, getattr(model, "config", None))
    logger.info("***** Running training *****")
    logger.info("  Num examples = %d", len(train_ds))
    logger.info("  Batch size = %d (x %d ranks of %d)", args.train_batch_size, world, per_rank)
    logger.info("  Num steps = %d", total)
    global_step = 0
    for epoch in range(int(args.start_epoch), int(args.num_train_epochs)):
        model.train()
        idx = iadist.shard_indices(len(train_ds), rank, world, args.seed + epoch, shuffle=True)
        # augmentation draws (data/transforms.py: the global `random`): a different stream per epoch and per rank, in the main
        # process (num_workers 0) and, through the loader's base seed, in every worker (base_seed + worker_id)
        aug_seed = (args.seed * 1000003 + epoch * 1009 + rank * 7919) & 0x7FFFFFFF
        random.seed(aug_seed)
        loader = DataLoader(Subset(train_ds, idx.tolist()), batch_size=per_rank, shuffle=False, collate_fn=collate_fn,
                            generator=torch.Generator().manual_seed(aug_seed), **feeder.loader_kw)
        opt.zero_grad()
        for step, batch in enumerate(loader):
            batch = feeder.decode_jpeg(batch)
            if batch is None:
                continue
            b = feeder.to_device(batch[2:])
            Fn.set_step_seed(ranks.seed(args.seed * 1000003 + global_step * 131 + step))
            loss = call_model(model, b).loss
            if step % args.log_steps == 0:
                logger.info(f"[Epoch-{epoch} Step-{step}] loss: {loss}")
            if accumulate_step(opt, loss, (step + 1) % args.gradient_accumulation_steps == 0, args.gradient_accumulation_steps,
                               linear_schedule_with_warmup(global_step, warm, total), reducer, average_grads):
                global_step += 1
        if args.do_eval and datasets.get("valid") is not None:
            logger.info(f"[Epoch-{epoch}] Starting evaluation ...")
            evaluate(args, model, datasets["valid"], collate_fn, call_model, feeder, ranks, f"Epoch-{epoch}")
        if rank == 0:
            logger.info(f"[Epoch-{epoch}] saving model")
            torch.save(model.state_dict(), os.path.join(out_dir, f"{checkpoint_name}_epoch-{epoch}.bin"))


def run(args, model, datasets, collate_fn, call_model, checkpoint_name, path_fields, device):
    """datasets: dict(train=..., valid=..., test=...) (entries may be None); call_model(model, batch) -> output where
    batch = collate output from index 2 on, already on `device`."""
    if getattr(args, "unpad", False):
        from .models import text as _text
        _text.UNPAD = True
    ranks = iadist.Ranks()
    try:
        ranks.init(device)
        out_dir = model_dir(args, path_fields)
        if ranks.rank == 0:
            os.makedirs(out_dir, exist_ok=True)
        feeder = BatchFeeder(args, device)
        if args.do_train:
            train_epochs(args, model, datasets, collate_fn, call_model, checkpoint_name, feeder, ranks, out_dir)
        elif args.do_eval and datasets.get("valid") is not None:
            evaluate(args, model, datasets["valid"], collate_fn, call_model, feeder, ranks, "Eval")
        if args.do_pred and datasets.get("test") is not None and ranks.rank == 0:
            predict(args, model, datasets["test"], collate_fn, call_model, feeder, out_dir)
        return out_dir
    finally:
        ranks.close()
