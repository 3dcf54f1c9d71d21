"""Domain-adaptive masked-LM + next-sentence pre-training of BertForPreTraining on the product corpus (reference bert_pretrain.py) on
the HIP engine.  The checkpoint it writes (`pytorch_model.bin`, `config.json`, `vocab.txt` under --output_dir) is what
`--pretrained_model_path` of finetune_text.py / finetune_multimodal.py starts the text towers from.

The reference hard-codes its settings in main(); each is a flag here whose default is the reference's value.  Kept as they are: the
schedule's length counts RECORDS, not examples (records // batch_size * num_epochs), and the next-sentence negatives are never trained
on (item_alignment_amd/data/bert_pretrain.py).  --model_name_or_path must be a local directory with vocab.txt and config.json (and
pytorch_model.bin to start from): nothing is ever downloaded.  INTEGRATION.md "BERT pre-training" has the details.

One process drives one GPU.  Under a launcher (python -m torch.distributed.run --nproc-per-node N bert_pretrain.py ...) the N ranks
train data-parallel: every rank runs the whole host pipeline from the same seed and so forms the one-process batches, takes its
contiguous slice of each, and the ranks together take the optimiser step of one process on the whole batch.  --batch_size stays the
total.  A batch with fewer rows than ranks is skipped by all ranks (the one departure from the one-process trajectory).  Rank 0 writes
the files.  Without WORLD_SIZE the script is the one-process script.
"""
import argparse
import logging
import os
import shutil
import sys

os.environ.setdefault("HF_HUB_OFFLINE", "1")
os.environ.setdefault("TRANSFORMERS_OFFLINE", "1")

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

LOGGER = logging.getLogger("bert_pretrain")


def get_parser():
    p = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    a = p.add_argument
    a("--data_dir", required=True, type=str, help="directory with the JSON-lines corpus files")
    a("--train_file", default="pretrain_train.jsonl", type=str)
    a("--valid_file", default="pretrain_valid.jsonl", type=str)
    a("--max_seq_len", default=510, type=int, help="tokens between [CLS] and [SEP]; the model sees max_seq_len + 2 positions")
    a("--batch_size", default=32, type=int, help="rows of one optimiser step; under a launcher the total over all ranks")
    a("--num_epochs", default=20, type=int)
    a("--model_name_or_path", required=True, type=str,
      help="LOCAL directory with vocab.txt, config.json and (optionally) pytorch_model.bin, e.g. an unpacked bert-base-chinese")
    a("--output_dir", default=os.path.join("src", "bert", "PretrainBert"), type=str)
    a("--learning_rate", default=2e-5, type=float)
    a("--adam_epsilon", default=1e-8, type=float)
    a("--warmup_steps", default=3000, type=int)
    a("--max_grad_norm", default=1.0, type=float)
    from item_alignment_amd.train import add_optimizer_flag
    add_optimizer_flag(p)
    a("--log_steps", default=100, type=int)
    a("--eval_steps", default=2000, type=int)
    a("--patience_steps", default=20000, type=int)
    a("--max_steps", default=-1, type=int, help="not in the reference: stop after this many optimiser steps (-1: run the epochs)")
    a("--seed", default=42, type=int, help="not in the reference: seeds the initialisation, the masking, the shuffles and the dropout")
    return p


def count_records(data_dir, file):
    with open(os.path.join(data_dir, file), "r", encoding="utf8") as f:
        return sum(1 for line in f if line.strip())


def main(argv=None):
    parser = get_parser()
    args = parser.parse_args(argv)
    from item_alignment_amd import dist as iadist
    ranks = iadist.Ranks()
    if args.batch_size % ranks.world:
        parser.error(f"--batch_size {args.batch_size} must be divisible by the world size {ranks.world}")
    from item_alignment_amd.cli_common import check_model_dir, rank0_run_logging
    check_model_dir(args.model_name_or_path)
    if ranks.rank == 0:                   # the log file, the scalars and the model directory are rank 0's alone
        os.makedirs(args.output_dir, exist_ok=True)
    with rank0_run_logging(LOGGER, ranks.rank, os.path.join(args.output_dir, "pretrain-bert.log"), os.path.join(args.output_dir, "tf-logs")) as writer:
        try:
            pretrain(args, ranks, writer)
        finally:
            ranks.close()
    return 0


def pretrain(args, ranks, writer):
    import torch
    import item_alignment_amd.models as M
    from item_alignment_amd import dist as iadist
    from item_alignment_amd.cli_common import linear_schedule, load_config, load_vocab_tokenizer
    from item_alignment_amd.data import bert_pretrain as D
    from item_alignment_amd.models import functional as Fn
    from item_alignment_amd.train import clipped_step
    clipped_optimizer_step = clipped_step(args)

    if not torch.cuda.is_available():
        raise SystemExit("bert_pretrain.py runs on the MI355X HIP engine only (no CPU path); no GPU is visible")
    device = ranks.init("cuda").device
    rank, world, dp = ranks.rank, ranks.world, ranks.dp

    vocab_file = os.path.join(args.model_name_or_path, "vocab.txt")
    tokenizer = load_vocab_tokenizer(vocab_file)
    config = load_config(os.path.join(args.model_name_or_path, "config.json"))
    if args.max_seq_len + 2 > config.max_position_embeddings:
        raise SystemExit(f"--max_seq_len {args.max_seq_len} + [CLS] + [SEP] exceeds max_position_embeddings {config.max_position_embeddings}")
    if len(tokenizer) > config.vocab_size:
        raise SystemExit(f"vocab.txt has {len(tokenizer)} entries, the model's word table {config.vocab_size} rows")
    torch.manual_seed(args.seed)
    model = M.BertForPreTraining.from_pretrained(args.model_name_or_path, config=config).to(device)
    LOGGER.info("The BERT model has {:} different named parameters.".format(len(list(model.named_parameters()))))
    arena = model.param_arena
    reducer = ranks.attach(arena)
    if dp:
        LOGGER.info(f"Data parallel: {world} ranks, --batch_size {args.batch_size} is the total ({args.batch_size // world} rows a rank)")
    rng = D.Rng(args.seed)            # the same seed on every rank: the same records, masking draws and shuffles, the same global batches

    total_steps = max(1, count_records(args.data_dir, args.train_file) // args.batch_size * args.num_epochs)
    eval_examples = []
    for records in D.read_pretrained_data(args.data_dir, args.valid_file, rng, batch_size=-1):
        eval_examples = D.build_examples(records, tokenizer, args.max_seq_len, rng)
    LOGGER.info(f"Loading Eval data successfully: {len(eval_examples)} examples")

    def run(batch, shares=None):
        input_ids, attention_mask, _token_type_ids, label_ids, next_labels = (b.to(device) for b in batch)
        # token_type_ids=None, as the reference calls its model: the segment types of the features are not fed in
        return model(input_ids, token_type_ids=None, attention_mask=attention_mask, masked_lm_labels=label_ids,
                     next_sentence_label=next_labels, loss_shares=shares)[0]

    def eval_model():
        """the mean of the per-batch losses (the reference's number).  Data parallel: rank r takes the whole batches i % world == r,
        the sum and the count are all-reduced, every rank holds the same mean"""
        model.eval()
        total, n = 0.0, 0
        with torch.no_grad():
            for i, batch in enumerate(D.batches(eval_examples, args.batch_size)):
                if i % world != rank:
                    continue
                total += run(batch).item()
                n += 1
        model.train()
        if dp:
            both = iadist.all_reduce_scalar(torch.tensor([total, n], dtype=torch.float64, device=device)).tolist()
            total, n = both[0], int(both[1])
        return total / max(1, n)

    def save():
        if rank == 0:
            model.save_pretrained(args.output_dir)
            shutil.copyfile(vocab_file, os.path.join(args.output_dir, "vocab.txt"))
        ranks.written()

    # the epochs; the function returns at early stopping and at --max_steps, on every rank at the same step
    global_steps, best_eval_loss, best_steps = 0, float("inf"), 0
    model.train()
    for epoch_idx in range(args.num_epochs):
        for records in D.read_pretrained_data(args.data_dir, args.train_file, rng):
            examples = D.build_examples(records, tokenizer, args.max_seq_len, rng)
            for whole in D.batches(examples, args.batch_size, rng):
                shares, inv_world = None, 1.0
                batch = ranks.cut(whole)
                if batch is None:             # global_steps does not move
                    LOGGER.info(f"Epoch {epoch_idx + 1}: a batch of {whole[0].shape[0]} rows skipped on every rank, fewer rows than the {world} ranks")
                    continue
                if dp:
                    # the masked-LM term is a mean over labelled rows, the next-sentence term a mean over rows: one count exchange
                    shares, _ = iadist.loss_shares([int((batch[3] != -1).sum()), batch[0].shape[0]])
                Fn.set_step_seed(ranks.seed(args.seed * 1000003 + global_steps))
                Fn.reset_use_counts()
                arena.zero_grad()
                loss = run(batch, shares)
                loss.backward()
                if reducer is not None:
                    inv_world = reducer.finish()
                global_steps += 1
                lr = args.learning_rate * linear_schedule(global_steps - 1, total_steps, args.warmup_steps)
                clipped_optimizer_step(arena, lr, args.max_grad_norm, inv_world, betas=(0.9, 0.999), eps=args.adam_epsilon, weight_decay=0.0)
                if global_steps % args.log_steps == 0:
                    # the weighted rank losses average to the loss of the global batch
                    value = ranks.mean(loss)
                    if writer:
                        writer.add_scalar("Train/loss", value, global_steps)
                    LOGGER.info("Epoch {:>3,}, Steps {:>5,}, Total {:>5,}, Train/Loss {:.6f}".format(epoch_idx + 1, global_steps, total_steps, value))
                if global_steps % args.eval_steps == 0:
                    eval_loss = eval_model()
                    if writer:
                        writer.add_scalar("Eval/loss", eval_loss, global_steps)
                    improve = "  No optimization! ..."
                    if best_eval_loss > eval_loss:
                        best_eval_loss, best_steps, improve = eval_loss, global_steps, " ^_^"
                        save()
                    elif global_steps - best_steps > args.patience_steps:
                        LOGGER.info(f"Eval loss has not been optimized for {args.patience_steps} steps, Early stopping ...")
                        LOGGER.info(f"Pretraining successfully, num_epochs:{epoch_idx + 1}, global_steps:{global_steps} ^_^")
                        return
                    LOGGER.info("* Epoch {:>3,}, Steps {:>5,}, Total {:>5,}, Eval/Loss {:.6f}".format(epoch_idx + 1, global_steps, total_steps,
                                                                                                   eval_loss) + improve)
                if 0 < args.max_steps <= global_steps:
                    LOGGER.info(f"Stopping after --max_steps {args.max_steps}")
                    return


if __name__ == "__main__":
    sys.exit(main())
