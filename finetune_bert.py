"""Fine-tunes the BERT pair classifier BertAlignModel (reference finetune_bert.py, "bert_base-one_tower-cls-NA-ce") on the HIP engine:
five fields of every product pair through one BERT encoder, a next-sentence head on the summed pooled outputs, cross-entropy.
It starts from a plain BERT directory or from the one bert_pretrain.py writes.

The reference hard-codes its settings in main(); each is a flag here whose default is the reference's value.  Kept as they are: the
best-F1 search skips the cut behind the last pair and reports a mid-point threshold; a checkpoint is written only inside an
evaluation; training stops early only when BOTH the evaluation loss and F1 have gone --patience_steps without improving.
Different: bert_align_results.csv goes to --output_dir and every row follows the header's column order;
classify F1 is 0.0 where the reference divides by zero; --model_name_or_path must be a local directory, nothing is ever downloaded;
the adversarial modes are not built; a resumed run goes on where the interrupted one stopped (same epoch, same batch) instead of
starting its epochs again.

One process drives one GPU.  Under a launcher (python -m torch.distributed.run --nproc-per-node N finetune_bert.py ...) the N ranks
train data-parallel: every rank builds the same loaders from the same seed, takes its contiguous slice of each global batch, and the
ranks together take the optimiser step of one process on the whole batch.  --batch_size stays the total.  A batch with fewer pairs
than ranks is skipped by all ranks (the one departure from the one-process trajectory).  Evaluation batches are dealt round-robin
and gathered, so every rank holds the one-process metrics; rank 0 writes the files.  Without WORLD_SIZE the script is the one-process
script.
"""
import argparse
import csv
import datetime
import os
import shutil
import sys
import time
from types import SimpleNamespace

os.environ.setdefault("HF_HUB_OFFLINE", "1")
os.environ.setdefault("TRANSFORMERS_OFFLINE", "1")

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

CSV_FILE = "bert_align_results.csv"
CSV_HEADERS = ["accuracy", "f1", "precision", "recall", "threshold", "classify_accuracy", "classify_f1", "classify_precision",
               "classify_recall", "classify_threshold", "epoch", "steps"]
BATCH_KEYS = [f"{field}_{kind}" for field in ("pvs", "title", "cate", "cate_path", "industry_name")
              for kind in ("input_ids", "attention_mask", "token_type_ids")]          # the loader's first fifteen tensors, in its order


def add_length_flags(a):
    a("--pvs_len", default=512, type=int)
    a("--title_len", default=150, type=int)
    a("--cate_len", default=20, type=int)
    a("--cate_path_len", default=50, type=int)
    a("--industry_name_len", default=20, type=int)


def get_parser():
    p = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    a = p.add_argument
    a("--data_dir", required=True, type=str, help="directory with the pair files")
    a("--output_dir", required=True, type=str)
    a("--train_file", default="item-align-train.json", type=str)
    a("--valid_file", default="item-align-val.json", type=str)
    a("--model_name_or_path", required=True, type=str,
      help="LOCAL directory with vocab.txt, config.json and (optionally) pytorch_model.bin: an unpacked bert-base-chinese, or the "
           "output directory of bert_pretrain.py")
    a("--restore_path", default="", type=str, help="a state_dict file loaded over the starting weights (keys may carry a module. prefix)")
    a("--batch_size", default=16, type=int, help="pairs of one optimiser step; under a launcher the total over all ranks")
    a("--num_epochs", default=20, type=int)
    a("--patience_steps", default=20000, type=int)
    a("--learning_rate", default=2e-5, type=float)
    a("--adam_epsilon", default=1e-8, type=float)
    a("--warmup_steps", default=3000, type=int)
    a("--max_grad_norm", default=1.0, type=float)
    from item_alignment_amd.train import add_optimizer_flag
    add_optimizer_flag(p)
    a("--log_steps", default=100, type=int)
    a("--eval_steps", default=1000, type=int)
    a("--check_steps", default=1000, type=int)
    add_length_flags(a)
    a("--shuffle_pvs", action="store_true", help="reorder the ;-separated pvs attributes of the training pairs and swap the two sides "
      "half of the time (the reference's shuffle_pvs, off in its main())")
    a("--seed", default=42, type=int, help="not in the reference: seeds the initialisation, the data order, the pvs shuffle and the dropout")
    a("--max_steps", default=-1, type=int, help="not in the reference: stop after this many optimiser steps (-1: run the epochs)")
    return p


def lengths_of(args):
    return dict(pvs_len=args.pvs_len, title_len=args.title_len, cate_len=args.cate_len, cate_path_len=args.cate_path_len,
                industry_name_len=args.industry_name_len)


def check_lengths(args, config):
    longest = max(lengths_of(args).values())
    if longest > config.max_position_embeddings:
        raise SystemExit(f"a field length of {longest} exceeds max_position_embeddings {config.max_position_embeddings}")


def load_pairs(data_dir, filename, batch_size, tokenizer, mode, lengths, shuffle_pvs=False, seed=0, generator=None):
    """pair file -> loader of the sixteen tensors (reference get_dataloader_from_files)"""
    from item_alignment_amd.data import bert_align as D
    pvs, title, industry_name, cate, cate_path = D.join_data(data_dir, filename, do_shuffle=shuffle_pvs, seed=seed)
    for rows, name in ((pvs, "pvs"), (title, "title"), (industry_name, "industry_name"), (cate, "cate"), (cate_path, "cate_path")):
        D.show(rows, mode, name)
    *cols, labels = D.get_examples(pvs, title, cate, cate_path, industry_name)
    D.LOGGER.info(f"======== Encode {mode} data ==========")
    enc = D.encode(tokenizer, *cols, **lengths)
    return D.get_dataloader(*enc, labels, batch_size=batch_size, mode=mode, generator=generator)


def load_state_file(model, path):
    """the reference's load_model: the keys the model has are taken from the file, with or without a `module.` prefix"""
    import torch
    own = model.state_dict()
    have = torch.load(path, map_location="cpu")
    picked = {}
    for key, value in have.items():
        bare = key[len("module."):] if key.startswith("module.") else key
        if bare in own:
            picked[bare] = value
    own.update(picked)
    model.load_state_dict(own)
    return len(picked)


def forward(model, batch, device, with_labels=True):
    d = [t.to(device) for t in batch]
    kw = dict(zip(BATCH_KEYS, d[:15]))
    return model(next_sentence_label=d[15] if with_labels else None, **kw), d[15]


def gather_in_batch_order(rows, width, device):
    """rows: this rank's records, each a tuple of `width` numbers whose first is the index of the evaluation batch it came from ->
    the records of all ranks, in the order one process produces them.  gather_shards concatenates rank-major and keeps every batch's
    records together and in order; a stable sort by the batch index then restores the file order.  fp64 carries fp32 logits, the
    labels and the indices exactly."""
    import torch
    from item_alignment_amd import dist as iadist
    local = torch.tensor(rows, dtype=torch.float64, device=device).reshape(-1, width)
    both = iadist.gather_shards(local)[0].cpu()
    return both[torch.argsort(both[:, 0], stable=True)].tolist()


def evaluate(model, loader, device, rank=0, world=1):
    """-> dict of the best-F1 search over logit[1] - logit[0], the argmax confusion figures and the mean loss (reference
    finetune_bert.py:129-181).  world > 1: rank r runs the batches i % world == r; the logits, labels and per-batch losses are
    gathered in the original order and every rank computes the metrics of one process from them."""
    import torch
    from item_alignment_amd.data import bert_align as D
    model.eval()
    rows, losses = [], []          # (batch, logit 0, logit 1, label) per pair; (batch, loss) per batch
    with torch.no_grad():
        for i, batch in enumerate(loader):
            if i % world != rank:
                continue
            out, labels = forward(model, batch, device)
            losses.append((i, out[-1].item()))
            rows += [(i, row[0], row[1], y) for row, y in zip(out[1].float().cpu().tolist(), labels.cpu().tolist())]
    if world > 1:
        rows, losses = gather_in_batch_order(rows, 4, device), gather_in_batch_order(losses, 2, device)
    total_loss, n = 0.0, len(losses)
    for _, value in losses:
        total_loss += value
    logits, truth = [[r[1], r[2]] for r in rows], [int(r[3]) for r in rows]
    tp, fp, tn, fn = D.confusion(logits, truth) if rows else (0, 0, 0, 0)
    scores = [row[1] - row[0] for row in logits]
    acc, f1, pre, recall, threshold = D.find_best_f1_and_threshold(scores, truth, True)
    cls_recall = tp / (tp + fn) if tp + fn else 0.0
    cls_pre = tp / (tp + fp) if tp + fp else 0.0
    cls_f1 = 2 * cls_pre * cls_recall / (cls_pre + cls_recall) if cls_pre + cls_recall else 0.0      # the reference divides by zero here
    return SimpleNamespace(acc=acc, f1=f1, pre=pre, recall=recall, threshold=threshold, cls_acc=(tp + tn) / max(1, tp + tn + fp + fn),
                           cls_f1=cls_f1, cls_pre=cls_pre, cls_recall=cls_recall, loss=total_loss / max(1, n))


def write_csv_row(output_dir, r, epoch, steps):
    path = os.path.join(output_dir, CSV_FILE)
    new = not os.path.isfile(path)
    with open(path, "w" if new else "a", newline="", encoding="utf-8") as f:
        w = csv.writer(f)
        if new:
            w.writerow(CSV_HEADERS)
        w.writerow([r.acc, r.f1, r.pre, r.recall, r.threshold, r.cls_acc, r.cls_f1, r.cls_pre, r.cls_recall, 0.5, epoch, steps])


def save_checkpoint(model, arena, global_steps, total_steps, args, path):
    """model_state_dict, optimizer_state_dict, scheduler_state_dict, global_steps -- the reference's four keys.  The optimiser is the
    arena's fused AdamW or LAMB (--optimizer, recorded by name): its state is the two moment buffers and the step count; the schedule
    is a function of the step."""
    import torch
    torch.save({
        "model_state_dict": {k: v.detach().cpu().clone() for k, v in model.state_dict().items()},
        "optimizer_state_dict": {"exp_avg": arena.exp_avg.cpu(), "exp_avg_sq": arena.exp_avg_sq.cpu(), "step": arena.step_count,
                                 "optimizer": args.optimizer, "names": list(arena.names), "offsets": list(arena.offsets)},
        "scheduler_state_dict": {"last_epoch": global_steps, "total_steps": total_steps, "warmup_steps": args.warmup_steps,
                                 "base_lr": args.learning_rate},
        "global_steps": global_steps,
    }, path)


def check_checkpoint_optimizer(state, args):
    """a checkpoint continues with the optimiser that wrote it (one written before the flag existed: adamw): the moments of the one
    are no state of the other"""
    saved = state.get("optimizer", "adamw")
    if saved != args.optimizer:
        raise SystemExit(f"the checkpoint was written with --optimizer {saved}: resuming it with --optimizer {args.optimizer} is refused "
                         "(pass the same optimiser, or start from --restore_path without the checkpoint)")


def restore_optimizer(arena, state):
    if list(state["names"]) != list(arena.names) or list(state["offsets"]) != list(arena.offsets):
        raise SystemExit("the checkpoint's optimiser state was written for another parameter layout")
    arena.exp_avg.copy_(state["exp_avg"])
    arena.exp_avg_sq.copy_(state["exp_avg_sq"])
    arena.step_count = int(state["step"])


def batch_size_error(args):
    """the message of the usage error where the launcher's world size does not divide --batch_size, or None"""
    from item_alignment_amd import dist as iadist
    world = iadist.env_ranks()[1]
    return f"--batch_size {args.batch_size} must be divisible by the world size {world}" if args.batch_size % world else None


def run(args):
    """the training run; returns what a caller may want to look at afterwards (the model, the step count)"""
    from item_alignment_amd import dist as iadist
    if batch_size_error(args):
        raise SystemExit(batch_size_error(args))
    ranks = iadist.Ranks()
    rank, world, dp = ranks.rank, ranks.world, ranks.dp
    from item_alignment_amd.cli_common import check_model_dir, linear_schedule, load_config, load_vocab_tokenizer, rank0_run_logging
    check_model_dir(args.model_name_or_path)
    import torch
    import item_alignment_amd.models as M
    from item_alignment_amd.data.bert_align import LOGGER
    from item_alignment_amd.models import functional as Fn
    from item_alignment_amd.train import clipped_step
    clipped_optimizer_step = clipped_step(args)

    config = load_config(os.path.join(args.model_name_or_path, "config.json"))
    check_lengths(args, config)
    if not torch.cuda.is_available():
        raise SystemExit("finetune_bert.py runs on the MI355X HIP engine only (no CPU path); no GPU is visible")
    loss_dir, f1_dir = os.path.join(args.output_dir, "LossModel"), os.path.join(args.output_dir, "F1Model")
    log_dir = os.path.join(args.output_dir, "tf-logs")
    checkpoint_path = os.path.join(args.output_dir, "checkpoint")
    try:
        device = ranks.init("cuda").device
        if rank == 0:                     # the directories, the log file, the scalars, the CSV and the models are rank 0's alone
            for d in (loss_dir, f1_dir, log_dir):
                os.makedirs(d, exist_ok=True)
        with rank0_run_logging(LOGGER, rank, os.path.join(log_dir, f"train-{datetime.date.today()}.log"), log_dir) as writer:
            def scalars(prefix, **values):
                if writer:
                    for k, v in values.items():
                        writer.add_scalar(f"{prefix}/{k}", v, global_steps)

            vocab_file = os.path.join(args.model_name_or_path, "vocab.txt")
            tokenizer = load_vocab_tokenizer(vocab_file)
            if len(tokenizer) > config.vocab_size:
                raise SystemExit(f"vocab.txt has {len(tokenizer)} entries, the model's word table {config.vocab_size} rows")
            lengths = lengths_of(args)
            order = torch.Generator()          # the training order of an epoch is a function of (seed, epoch) alone: a resumed run finds it again
            train_loader = load_pairs(args.data_dir, args.train_file, args.batch_size, tokenizer, "train", lengths, args.shuffle_pvs, args.seed,
                                      order)
            eval_loader = load_pairs(args.data_dir, args.valid_file, args.batch_size, tokenizer, "eval", lengths)

            torch.manual_seed(args.seed)
            model = M.BertAlignModel.from_pretrained(args.model_name_or_path, config=config)
            if args.restore_path:
                LOGGER.info(f"Loaded {load_state_file(model, args.restore_path)} tensors from {args.restore_path}")
            else:
                LOGGER.info("There is no restore model path.")
            global_steps, optimizer_state = 0, None
            if os.path.exists(checkpoint_path):
                ck = torch.load(checkpoint_path, map_location="cpu")
                model.load_state_dict({(k[len("module."):] if k.startswith("module.") else k): v for k, v in ck["model_state_dict"].items()})
                global_steps, optimizer_state = int(ck["global_steps"]), ck["optimizer_state_dict"]
                check_checkpoint_optimizer(optimizer_state, args)
                del ck
            else:
                LOGGER.info("There is no resume model path.")
            model.to(device)
            arena = model.param_arena
            if optimizer_state is not None:
                restore_optimizer(arena, optimizer_state)
                LOGGER.info(f"Load checkpoint from {checkpoint_path} successfully: resumed at global_steps {global_steps}, train continue ...")
            LOGGER.info("The BERT model has {:} different named parameters.".format(len(list(model.named_parameters()))))
            reducer = ranks.attach(arena)          # after the weights and the checkpoint (every rank has also read the moments itself)
            if dp:
                LOGGER.info(f"Data parallel: {world} ranks, --batch_size {args.batch_size} is the total ({args.batch_size // world} pairs a rank)")

            per_epoch = len(train_loader)
            total_steps = max(1, per_epoch * args.num_epochs)
            best_f1, best_eval_loss = 0.0, float("inf")
            best_loss_steps = best_f1_steps = global_steps
            t0 = time.time()

            def save_model(directory):
                if rank == 0:
                    model.save_pretrained(directory)
                    shutil.copyfile(vocab_file, os.path.join(directory, "vocab.txt"))
                    LOGGER.info(f"* Save model to {directory}")
                ranks.written()

            def done():
                return SimpleNamespace(model=model, global_steps=global_steps, best_f1=best_f1, best_eval_loss=best_eval_loss)

            # global_steps counts global batches.  Several ranks skip an epoch's last batch where it has fewer pairs than ranks: that epoch
            # then has one step less than batches (the skipped batch is its last, so batch index and step count still agree inside it)
            tail = len(train_loader.dataset) % args.batch_size
            steps_per_epoch = per_epoch - (1 if dp and 0 < tail < world else 0)
            first_epoch, skip = divmod(global_steps, max(1, steps_per_epoch))
            if 0 < args.max_steps <= global_steps:
                LOGGER.info(f"--max_steps {args.max_steps} was reached before this run")
                return done()
            for epoch in range(first_epoch, args.num_epochs):
                LOGGER.info("======== Training Epoch {:} / {:} ========".format(epoch + 1, args.num_epochs))
                model.train()
                order.manual_seed(args.seed * 1000003 + epoch)
                for step, whole in enumerate(train_loader):
                    if epoch == first_epoch and step < skip:          # the batches the interrupted run had already trained on
                        continue
                    inv_world = 1.0
                    batch = ranks.cut(whole)
                    if batch is None:             # global_steps does not move
                        LOGGER.info(f"Epoch {epoch + 1}: a batch of {whole[0].shape[0]} pairs skipped on every rank, fewer pairs than the {world} ranks")
                        continue
                    Fn.set_step_seed(ranks.seed(args.seed * 1000003 + global_steps))
                    Fn.reset_use_counts()
                    arena.zero_grad()
                    loss = forward(model, batch, device)[0][-1]
                    if dp:                    # the mean over this rank's pairs, weighted by its share of the global batch's pairs
                        loss = loss * iadist.loss_shares([batch[0].shape[0]])[0][0]
                    loss.backward()
                    if reducer is not None:
                        inv_world = reducer.finish()
                    global_steps += 1
                    lr = args.learning_rate * linear_schedule(global_steps - 1, total_steps, args.warmup_steps)
                    clipped_optimizer_step(arena, lr, args.max_grad_norm, inv_world, betas=(0.9, 0.999), eps=args.adam_epsilon, weight_decay=0.0)
                    if global_steps % args.log_steps == 0:
                        value = ranks.mean(loss)          # the weighted rank losses average to the loss of the global batch
                        scalars("Train", Loss=value)
                        LOGGER.info("Epoch {:>3,} - Steps {:>5,} - Total {:>5,} - Train/Loss {:.6f} - Total cost: {:}".format(
                            epoch + 1, global_steps, per_epoch, value, datetime.timedelta(seconds=int(time.time() - t0))))
                    if global_steps % args.eval_steps == 0:
                        LOGGER.info("======== Running Eval ========")
                        r = evaluate(model, eval_loader, device, rank, world)
                        if rank == 0:
                            write_csv_row(args.output_dir, r, epoch + 1, global_steps)
                        scalars("Eval", Acc=r.acc, Precision=r.pre, Recall=r.recall, F1=r.f1, cls_Acc=r.cls_acc, cls_Precision=r.cls_pre,
                                cls_Recall=r.cls_recall, cls_F1=r.cls_f1, Loss=r.loss)
                        LOGGER.info("* Epoch: {:>3,}, Steps {:>5,}, Accuracy: {:.4f}, Precision: {:.4f}, Recall: {:.4f}, F1: {:.4f}, Eval/Loss: {:.6f}"
                                    .format(epoch + 1, global_steps, r.acc, r.pre, r.recall, r.f1, r.loss))
                        LOGGER.info("* CLS Epoch: {:>3,}, Steps {:>5,}, Accuracy: {:.4f}, Precision: {:.4f}, Recall: {:.4f}, F1: {:.4f}"
                                    .format(epoch + 1, global_steps, r.cls_acc, r.cls_pre, r.cls_recall, r.cls_f1))
                        improved = []
                        if best_eval_loss > r.loss:
                            best_eval_loss, best_loss_steps = r.loss, global_steps
                            save_model(loss_dir)
                            improved.append("Eval/Loss")
                            LOGGER.info(f"* Current Best Eval/Loss {best_eval_loss} epoch:{epoch + 1}, steps:{global_steps}")
                        if best_f1 < r.f1:
                            best_f1, best_f1_steps = r.f1, global_steps
                            save_model(f1_dir)
                            improved.append("F1")
                            LOGGER.info(f"* Current Best F1 {best_f1} epoch:{epoch + 1}, steps:{global_steps} Eval/Loss:{r.loss}")
                        if global_steps % args.check_steps == 0:
                            if rank == 0:
                                save_checkpoint(model, arena, global_steps, total_steps, args, checkpoint_path)
                                LOGGER.info(f"* Save checkpoint to {checkpoint_path} .")
                            ranks.written()
                        if global_steps - best_loss_steps >= args.patience_steps and global_steps - best_f1_steps >= args.patience_steps:
                            LOGGER.info(f"There is no optimizing model after {max(global_steps - best_loss_steps, global_steps - best_f1_steps)} "
                                        "steps, Early stopping ....")
                            LOGGER.info(f"* Best F1 {best_f1} after {epoch + 1} epochs, {global_steps} steps training.")
                            return done()
                        model.train()
                        LOGGER.info((("Optimize " + " and ".join(improved)) if improved else "No optimization") + ", continue training ...")
                    if 0 < args.max_steps <= global_steps:
                        LOGGER.info(f"Stopping after --max_steps {args.max_steps}")
                        return done()
            LOGGER.info("Training successfully.")
            return done()
    finally:
        ranks.close()


def main(argv=None):
    parser = get_parser()
    args = parser.parse_args(argv)
    if batch_size_error(args):
        parser.error(batch_size_error(args))
    run(args)
    return 0


if __name__ == "__main__":
    sys.exit(main())
