#!/usr/bin/env python3
"""CoCa pre-training (reference coca_pretrain.py) on the HIP engine: CoCaForPretraining -- a RoBERTa text tower, a ViT, causal
multimodal layers -- trained on (title [+ attributes], image) items with a caption loss and a contrastive loss.  Each epoch writes
<output_dir>/<model_name>/coca_pretrain_epoch-{e}.bin, whose `coca.*` and `multimodal_layers.*` tensors are what
finetune_multimodal.py --ensemble cross_attn starts from (--file_state_dict).

Flags and defaults are the reference's; --max_steps and --num_workers are added.  Two things differ on purpose (notes
N2 and N3): the labels of the caption loss are input_ids[:, 1:] (the reference's [:, 2:] cannot run), and gradients accumulate over
--gradient_accumulation_steps micro-batches (the reference clears them at every micro-step).  The ViT's geometry comes from the config
file (patch_size, hidden_size, num_hidden_layers, num_attention_heads), as the reference's ViT(config) takes it; its weights from
image_encoder.bin under --pretrained_image_model_path.

One process drives one GPU.  Under a launcher (python -m torch.distributed.run --nproc-per-node N coca_pretrain.py ...) the N ranks
train data-parallel on one global batch: --train_batch_size stays the total, every rank takes 1/N of it, every item of the other
ranks is a contrastive negative (CoCaForPretraining.set_data_parallel), gradients are averaged in overlapped buckets
and rank 0 writes the files.  Without WORLD_SIZE the script is the one-process script.
"""
import argparse
import json
import os
import random
import sys

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def get_parser():
    p = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    a = p.add_argument
    a("--data_dir", required=True, type=str, help="模型训练数据地址: item_info.jsonl and item_images/")
    a("--output_dir", required=True, type=str, help="The output directory where the model checkpoints will be written.")
    a("--model_name", required=True, type=str, help="model name")
    a("--config_file", required=True, type=str, help="model config file (a path, or a name under --output_dir as in the reference)")
    a("--pretrained_text_model_path", required=True, type=str, help="pretrained text model path, RoBerta")
    a("--pretrained_image_model_path", required=True, type=str, help="pretrained image model path, ViT (a directory with image_encoder.bin, or the file)")
    # training
    a("--seed", default=2345, type=int, help="random seed")
    a("--train_batch_size", default=64, type=int, help="Total batch size for training.")
    a("--learning_rate", default=1e-3, type=float, help="The initial learning rate for Adam.")
    a("--start_epoch", default=0, type=int, help="starting training epoch")
    a("--num_train_epochs", default=1000, type=int, help="Total number of training epochs to perform.")
    a("--weight_decay", default=1e-5, type=float, help="weight decay")
    a("--log_steps", default=None, type=int, help="every n steps, log training process")
    a("--file_state_dict", default=None, type=str, help="finetuned model path")
    a("--parameters_to_freeze", default=None, type=str, help="file that contains parameters that do not require gradient descend")
    # optimization
    a("--warmup_proportion", default=0.1, type=float, help="Proportion of training to perform linear learning rate warmup for.")
    a("--gradient_accumulation_steps", default=1, type=int, help="Number of micro-batches accumulated into one optimiser step.")
    a("--adam_epsilon", default=1e-8, type=float, help="Epsilon for Adam optimizer.")
    a("--fp16", action="store_true", help="kept for CLI compatibility: the HIP engine always computes in bf16 with fp32 master weights")
    # cv
    a("--image_model_name", default="vit_base_patch16_384", type=str, help="image model name (unused, as in the reference: the config sets the ViT)")
    a("--image_size", default=384, type=int, help="image height and width in pixels")
    a("--hflip", default=0.5, type=float, help="image transform: horizontal flip")
    a("--color_jitter", default=None, type=float, help="image transform: color jitter")
    # NLP
    a("--do_lower_case", default=True, type=bool, help="Whether to lower case the input text.")
    a("--max_seq_len", default=None, type=int, help="max length for one item title")
    a("--max_seq_len_pv", default=None, type=int, help="max length of pvs, 'None' - do not add pvs as text")
    # Coca
    a("--caption_loss_weight", default=1.0, type=float, help="caption loss weight")
    a("--contrastive_loss_weight", default=1.0, type=float, help="constrative loss weight")
    # not in the reference
    a("--max_steps", default=-1, type=int, help="not in the reference: stop after this many optimiser steps (-1: run the epochs)")
    a("--num_workers", default=0, type=int, help="not in the reference: DataLoader worker processes for decode / tokenisation")
    return p


def load_raw_data(args):
    """reference coca_pretrain.py:70-97: (item_id, segmented title, segmented attributes, image path) per line of item_info.jsonl"""
    from item_alignment_amd.data.datasets import _cut
    from item_alignment_amd.utils import logger
    data = []
    with open(os.path.join(args.data_dir, "item_info.jsonl"), "r", encoding="utf-8") as r:
        for line in r:
            if not line.strip():
                continue
            d = json.loads(line)
            item_pvs, sku_pvs = d.get("item_pvs", "").replace("#", ""), d.get("sku_pvs", "").replace("#", "")
            pvs = ";".join(p for p in (item_pvs, sku_pvs) if len(p) > 0)
            data.append((d["item_id"], _cut(d.get("title", "")), _cut(pvs), os.path.join(args.data_dir, "item_images", d.get("item_image_name", ""))))
    logger.info(f"Finished load item info, size: {len(data)}")
    return data


def collate_or_none(inputs):
    """collate_coca, or None where every item of the micro-batch lost its image (a rank's share may be that small)"""
    from item_alignment_amd.data.datasets import collate_coca
    if not any(i.get("image") is not None for i in inputs):
        return None
    return collate_coca(inputs)


def main(argv=None):
    args = get_parser().parse_args(argv)
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("this model runs on the MI355X HIP engine only (no CPU path); no GPU is visible")
    from types import SimpleNamespace

    from torch.utils.data import DataLoader, Subset

    from item_alignment_amd import dist as iadist
    from item_alignment_amd import train
    from item_alignment_amd.cli_common import freeze_and_resume, load_config, load_tokenizer
    from item_alignment_amd.data.datasets import MultimodalDataset, collate_coca
    from item_alignment_amd.models import CoCaForPretraining, RobertaModel, VisionTransformer
    from item_alignment_amd.models import functional as Fn
    from item_alignment_amd.utils import VIT_WEIGHTS_NAME, logger

    ranks = iadist.Ranks()
    try:
        device = ranks.init("cuda").device
        rank, world, dp = ranks.rank, ranks.world, ranks.dp
        per_rank = args.train_batch_size // world
        if per_rank * world != args.train_batch_size:
            raise ValueError(f"--train_batch_size {args.train_batch_size} must be divisible by the world size {world}")
        logger.info(f"device: {device}, 16-bits training: {args.fp16} (ignored: bf16 activations, fp32 master weights)")
        train.seed_everything(args.seed)

        tokenizer = load_tokenizer(SimpleNamespace(pretrained_model_path=args.pretrained_text_model_path, do_lower_case=args.do_lower_case))
        config_file = args.config_file if os.path.isfile(args.config_file) else os.path.join(args.output_dir, args.config_file)
        config = load_config(config_file, image_size=args.image_size, max_seq_len=args.max_seq_len, max_seq_len_pv=args.max_seq_len_pv,
                             caption_loss_weight=args.caption_loss_weight, contrastive_loss_weight=args.contrastive_loss_weight)

        text_encoder = RobertaModel.from_pretrained(args.pretrained_text_model_path, config=config)
        image_encoder = VisionTransformer(img_size=args.image_size, patch_size=getattr(config, "patch_size", 16), embed_dim=config.hidden_size,
                                          depth=config.num_hidden_layers, num_heads=config.num_attention_heads)
        f = args.pretrained_image_model_path
        f = os.path.join(f, VIT_WEIGHTS_NAME) if os.path.isdir(f) else f
        if os.path.exists(f):
            image_encoder.load_state_dict(torch.load(f, map_location="cpu"), strict=False)
        else:
            logger.warning(f"{f} not found: the image encoder keeps its random initialisation (no network for timm weights)")
        model = CoCaForPretraining(config, text_encoder=text_encoder, image_encoder=image_encoder)
        freeze_and_resume(args, model)

        train_data = load_raw_data(args)
        logger.info(f"# train samples: {len(train_data)}")
        dataset = MultimodalDataset(train_data, image_size=args.image_size, is_training=True, text_tokenizer=tokenizer,
                                    max_seq_len=args.max_seq_len, max_seq_len_pv=args.max_seq_len_pv, hflip=args.hflip,
                                    color_jitter=args.color_jitter)
        model.to(device)
        opt = train.ArenaAdamW(model, args.learning_rate, args.adam_epsilon, args.weight_decay)
        total = int(len(dataset) / args.train_batch_size / args.gradient_accumulation_steps) * (args.num_train_epochs - args.start_epoch)
        warm = int(total * args.warmup_proportion)

        reducer = ranks.attach(model.param_arena)
        if dp:
            model.set_data_parallel()          # every item of the other ranks is a contrastive negative

        out_dir = os.path.join(args.output_dir, args.model_name)
        os.makedirs(out_dir, exist_ok=True)
        if rank == 0:
            train.dump_hyperparameters(out_dir, args, config)

        logger.info("***** Running training *****")
        logger.info("  Model name = %s", args.model_name)
        logger.info("  Num examples = %d", len(dataset))
        logger.info("  Batch size = %d", args.train_batch_size)
        if dp:
            logger.info("  Ranks = %d of %d items each (this is rank %d)", world, per_rank, rank)
        logger.info("  Num steps = %d", total)
        logger.info("  Learning rate = %.3f", args.learning_rate)

        global_step = 0
        for epoch in range(int(args.start_epoch), int(args.num_train_epochs)):
            model.train()
            # the shuffle and the augmentation draws depend on (seed, epoch) alone: a run resumed at --start_epoch sees that epoch's batches
            epoch_seed = (args.seed * 1000003 + epoch * 1009) & 0x7FFFFFFF
            random.seed(epoch_seed)
            if dp:
                # every rank takes positions rank::world of the epoch's permutation: equal shares, the same global order at any world size.
                # The augmentation draws differ per rank (item_alignment_amd/train.py): the ranks hold different items of one batch
                idx = iadist.shard_indices(len(dataset), rank, world, epoch_seed, shuffle=True)
                aug_seed = (args.seed * 1000003 + epoch * 1009 + rank * 7919) & 0x7FFFFFFF
                random.seed(aug_seed)
                loader = DataLoader(Subset(dataset, idx.tolist()), batch_size=per_rank, shuffle=False, collate_fn=collate_or_none,
                                    num_workers=args.num_workers, generator=torch.Generator().manual_seed(aug_seed))
            else:
                loader = DataLoader(dataset, batch_size=args.train_batch_size, shuffle=True, collate_fn=collate_coca, num_workers=args.num_workers,
                                    generator=torch.Generator().manual_seed(epoch_seed))
            opt.zero_grad()
            micro = 0           # micro-batches run since the epoch began; in one process every step is one
            for step, batch in enumerate(loader):
                if dp:
                    # the collate drops items whose image failed to load, so the ranks can arrive with different counts.  A rank without an
                    # item has nothing to put into the collectives of the step: every rank skips the micro-batch together
                    counts = [c[0] for c in iadist.gather_ints([0 if batch is None else len(batch[0])])]
                    if min(counts) == 0:
                        if rank == 0:
                            logger.info(f"[Epoch-{epoch} Step-{step}] skipped on every rank: item counts {counts}, a rank has none")
                        continue
                input_ids, attention_mask, token_type_ids, position_ids, images = (t.to(device, non_blocking=True) for t in batch[1:])
                Fn.set_step_seed(ranks.seed(args.seed * 1000003 + global_step * 131 + step))
                Fn.reset_use_counts()
                loss = model(input_ids, attention_mask, token_type_ids, position_ids, images)
                if args.log_steps is not None and step % args.log_steps == 0:
                    shown = ranks.mean(loss, in_dtype=True)          # the mean of the ranks' losses is the loss of the global batch
                    if rank == 0:
                        logger.info(f"[Epoch-{epoch} Step-{step}] loss: {shown:.6f}")
                micro += 1
                # the micro-batches of one optimiser step accumulate (note N3)
                if train.accumulate_step(opt, loss, micro % args.gradient_accumulation_steps == 0, args.gradient_accumulation_steps,
                                         train.linear_schedule_with_warmup(global_step, warm, total), reducer):
                    global_step += 1
                    if 0 < args.max_steps <= global_step:
                        break
            if rank == 0:
                logger.info(f"[Epoch-{epoch}] saving model ({global_step} optimiser steps so far)")
                sd = {k: v.detach().to("cpu", torch.float32 if v.is_floating_point() else v.dtype).clone() for k, v in model.state_dict().items()}
                torch.save(sd, os.path.join(out_dir, f"coca_pretrain_epoch-{epoch}.bin"))
            ranks.written()
            if 0 < args.max_steps <= global_step:
                logger.info(f"Stopping after --max_steps {args.max_steps}")
                break
    finally:
        ranks.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
