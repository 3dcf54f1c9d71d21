"""Graph two-tower fine-tuning on the MI355X HIP engine: the reference's finetune_graph.py (README 5.3.1) -- a GCNII encoder over
the item / attribute-value graph, TwoTowerClassificationHead on the node embeddings of a pair.  Same flags, defaults, input files,
output directory name, hyperparamter.txt, graph_epoch-{e}.bin checkpoints, P/R/F1 log lines and prediction jsonl.

Differences, all deliberate: the tokenizer the reference loads and never uses is not loaded (--pretrained_model_path is accepted and
ignored); --log_steps None (the default) skips the loss log line instead of failing on `step % None` (quirk G2); the optimiser is
the fused AdamW over the parameter arena; one GPU only -- every batch runs the whole graph, so data parallelism would only split
the pairs.  IA_GCN_PAIRWISE_LOSS=1 replaces the reference's pair-0 loss (quirk G1) by the per-pair one.
"""
import argparse
import json
import os

import numpy as np
import torch
from torch.utils.data import DataLoader

from item_alignment_amd import cli_common, train as T
from item_alignment_amd.utils import logger


def build_parser():
    parser = argparse.ArgumentParser()
    a = parser.add_argument
    # Required parameters
    a("--data_dir", required=True, type=str, help="模型训练数据地址")
    a("--output_dir", required=True, type=str, help="The output directory where the model checkpoints will be written.")
    a("--config_file", required=True, type=str, help="The config file which specified the model details.")
    a("--model_name", required=True, type=str, help="model saving name")
    a("--data_version", required=True, type=str, help="data version")
    a("--interaction_type", required=True, type=str, help="交互方式, one_tower: 中间过程有交互, two_tower: 中间过程无交互，最后embedding交互")
    a("--classification_method", required=True, type=str, help="分类方法, cls / vec_sim")
    a("--similarity_measure", required=True, type=str, help="向量相似度量: cosine, inner_product, l1, l2")
    a("--loss_type", required=True, type=str, help="损失函数类型 (the graph model reaches its loss with ce only)")
    # training
    a("--do_train", action="store_true", help="是否进行模型训练")
    a("--do_eval", action="store_true", help="是否进行模型验证")
    a("--do_pred", action="store_true", help="是否进行模型测试")
    a("--seed", default=2345, type=int, help="random seed")
    a("--train_batch_size", default=512, type=int, help="Total batch size for training.")
    a("--eval_batch_size", default=1024, type=int, help="Total batch size for evaluation.")
    a("--learning_rate", default=1e-3, type=float, help="The initial learning rate for Adam.")
    a("--start_epoch", default=0, type=int, help="starting training epoch")
    a("--num_train_epochs", default=500, type=int, help="Total number of training epochs to perform.")
    a("--weight_decay", default=1e-5, type=float, help="weight decay")
    a("--log_steps", default=None, type=int, help="every n steps, log training process")
    a("--save_epochs", default=10, type=int, help="every n epochs, save model and eval")
    a("--pretrained_model_path", default=None, type=str, help="accepted for compatibility; the graph model loads no tokenizer")
    a("--file_state_dict", default=None, type=str, help="finetuned model path")
    a("--parameters_to_freeze", default=None, type=str, help="file that contains parameters that do not require gradient descend")
    a("--threshold", default=0.5, type=float, help="default threshold for item embedding score for prediction")
    # optimization
    a("--warmup_proportion", default=0.1, type=float, help="Proportion of training to perform linear learning rate warmup for.")
    a("--gradient_accumulation_steps", default=1, type=int, help="Number of updates steps to accumualte before performing a backward/update pass.")
    a("--adam_epsilon", default=1e-8, type=float, help="Epsilon for Adam optimizer.")
    a("--fp16", action="store_true", help="kept for CLI compatibility: the graph kernels compute in fp32")
    a("--margin", default=1.0, type=float, help="margin in loss function")
    # NLP
    a("--do_lower_case", default=True, type=bool, help="unused (no tokenizer is loaded)")
    # GNN
    a("--num_layers", default=4, type=int, help="number of gcn layers")
    a("--hidden_size", default=128, type=int, help="gcn hidden_size")
    a("--feature_dim", default=1024, type=int, help="feature matrix dim (equal to roberta large hidden size)")
    a("--alpha", default=0.1, type=float, help="gcn layer param")
    a("--theta", default=0.5, type=float, help="gcn layer param")
    return parser


def get_parser(argv=None):
    return build_parser().parse_args(argv)


def load_raw_data(args):
    """reference finetune_graph.py:73-123."""
    e2id = {}
    with open(os.path.join(args.data_dir, "processed", "entity2id.txt"), "r", encoding="utf-8") as r:
        for line in r:
            if not line.strip("\n"):
                continue
            k, v = line.strip("\n").split("\t")
            if "/item/" in k:
                e2id[k.replace("/item/", "")] = int(v)

    def pairs(name):
        out = []
        with open(os.path.join(args.data_dir, "raw", name), "r", encoding="utf-8") as r:
            for line in r:
                if not line.strip():
                    continue
                d = json.loads(line)
                d["src_idx"], d["tgt_idx"] = e2id[d["src_item_id"]], e2id[d["tgt_item_id"]]
                out.append(d)
        return out

    return pairs("item_train_train_pair.jsonl"), pairs("item_train_valid_pair.jsonl"), pairs("item_valid_pair.jsonl")


def evaluate(model, loader, feature_matrix, adj, tag):
    """reference finetune_graph.py:364-426: P / R / F1 swept over the thresholds 0.1 .. 0.9."""
    model.eval()
    probs_all, labels_all = None, None
    with torch.no_grad():
        for batch in loader:
            labels = np.array([int(b["item_label"]) for b in batch])
            probs = model(feature_matrix=feature_matrix, adjacency_matrix=adj, pairs=batch).probs.cpu().numpy()
            probs_all = probs if probs_all is None else np.append(probs_all, probs)
            labels_all = labels if labels_all is None else np.append(labels_all, labels)
    T.log_threshold_sweep(probs_all, labels_all, tag)


def main(argv=None):
    args = get_parser(argv)
    if int(os.environ.get("WORLD_SIZE", "1")) > 1:
        raise SystemExit("finetune_graph.py runs on one GPU: every batch is a forward and backward over the whole graph, the same on "
                         "every rank, so data parallelism would only split the pairs of a batch (WORLD_SIZE must be 1)")
    T.seed_everything(args.seed)
    config = cli_common.load_config(os.path.join(args.output_dir, args.config_file), interaction_type=args.interaction_type,
                                    classification_method=args.classification_method, similarity_measure=args.similarity_measure,
                                    loss_type=args.loss_type, intermediate_size=args.hidden_size, num_hidden_layers=args.num_layers,
                                    hidden_size=args.feature_dim, alpha=args.alpha, theta=args.theta)
    from item_alignment_amd.data.datasets import GCNDataset, collate_gnn
    from item_alignment_amd.models import GCNTwoTower, load_adjacency
    from item_alignment_amd.models import functional as Fn
    if "gcn" in args.model_name:
        model = GCNTwoTower(config=config)
    else:
        raise ValueError("model name should be: gcn")
    cli_common.freeze_and_resume(args, model)
    train_data, valid_data, test_data = load_raw_data(args)
    logger.info(f"# train samples: {len(train_data)}, # valid samples: {len(valid_data)}, # test samples: {len(test_data)}")
    device = cli_common.pick_device(model)
    model.to(device)
    adj = load_adjacency(torch.load(os.path.join(args.data_dir, "processed", "adj_t.pt"), map_location="cpu", weights_only=False), device=device)
    feature_matrix = torch.load(os.path.join(args.data_dir, "processed", "feature_matrix.pt"), map_location="cpu",
                                weights_only=False).to(device=device, dtype=torch.float32)
    logger.info(f"graph: {adj.num_nodes} nodes, {adj.nnz} edges, features {tuple(feature_matrix.shape)}")

    out_dir = T.model_dir(args, ("model_name", "data_version", "interaction_type", "classification_method", "similarity_measure", "loss_type"))
    os.makedirs(out_dir, exist_ok=True)
    valid_loader = DataLoader(GCNDataset(valid_data), batch_size=args.eval_batch_size, shuffle=False, collate_fn=collate_gnn) if args.do_eval else None

    if args.do_train:
        train_ds = GCNDataset(train_data)
        loader = DataLoader(train_ds, batch_size=args.train_batch_size, shuffle=True, collate_fn=collate_gnn,
                            generator=torch.Generator().manual_seed(args.seed))
        opt = T.ArenaAdamW(model, args.learning_rate, args.adam_epsilon, args.weight_decay)
        total = int(len(train_ds) / args.train_batch_size / args.gradient_accumulation_steps) * (args.num_train_epochs - args.start_epoch)
        warm = int(total * args.warmup_proportion)
        T.dump_hyperparameters(out_dir, args, config)
        logger.info("***** Running training *****")
        logger.info("  Model name = %s", os.path.basename(out_dir))
        logger.info("  Num examples = %d", len(train_ds))
        logger.info("  Batch size = %d", args.train_batch_size)
        logger.info("  Num steps = %d", total)
        logger.info("  Learning rate = %.5f", args.learning_rate)
        global_step = 0
        for epoch in range(int(args.start_epoch), int(args.num_train_epochs)):
            model.train()
            opt.zero_grad()
            losses = []
            for step, batch in enumerate(loader):
                Fn.set_step_seed((args.seed * 1000003 + global_step * 131 + step) & 0xFFFFFFFF)
                output = model(feature_matrix=feature_matrix, adjacency_matrix=adj, pairs=batch)
                loss = output.loss
                losses.append(loss.detach())
                if args.log_steps is not None and step % args.log_steps == 0:
                    logger.info(f"[Epoch-{epoch} Step-{step}] loss: {loss}")
                if T.accumulate_step(opt, loss, (step + 1) % args.gradient_accumulation_steps == 0, args.gradient_accumulation_steps,
                                     T.linear_schedule_with_warmup(global_step, warm, total)):
                    global_step += 1
            logger.info(f"[Epoch-{epoch}] mean training loss: {float(torch.stack(losses).mean())}")
            if args.save_epochs is not None and epoch % args.save_epochs == 0:
                if args.do_eval:
                    logger.info(f"[Epoch-{epoch}] Starting evaluation ...")
                    evaluate(model, valid_loader, feature_matrix, adj, f"[Epoch-{epoch}] ")
                logger.info(f"[Epoch-{epoch}] saving model")
                torch.save(model.state_dict(), os.path.join(out_dir, f"graph_epoch-{epoch}.bin"))
    elif args.do_eval:
        evaluate(model, valid_loader, feature_matrix, adj, "")

    if args.do_pred:
        model.eval()
        test_loader = DataLoader(GCNDataset(test_data), batch_size=args.eval_batch_size, shuffle=False, collate_fn=collate_gnn)

        def rows_of(batch):
            output = model(feature_matrix=feature_matrix, adjacency_matrix=adj, pairs=batch)
            return [b["src_item_id"] for b in batch], [b["tgt_item_id"] for b in batch], output.src_embeds.cpu().numpy(), output.tgt_embeds.cpu().numpy()

        T.write_pair_embeddings(os.path.join(out_dir, f"deepAI_result_threshold={args.threshold}.jsonl"), test_loader, rows_of, args.threshold,
                                args.log_steps)
    return out_dir


if __name__ == "__main__":
    main()
