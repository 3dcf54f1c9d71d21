#!/usr/bin/env python3
"""Node features for the graph two-tower: the RoBERTa pooler output of every entity of the knowledge graph, written to
processed/feature_matrix.pt -- the reference's pred_text.py (flags :19-62, input :65-93, loop :155-192) on the MI355X HIP engine.

Every line of processed/entity2id.txt becomes one text: `/item/<id>` the title of that item in raw/item_info.jsonl, `/value/<v>` the
string v.  The texts go through the text tower forward-only (ia_layer_fwd_infer; the last layer runs for the [CLS] rows alone) and the
pooler, tanh(dense(h[CLS])); row k of the saved fp32 [N, H] matrix is line k of the file.

Deviations from the reference, all deliberate: --pretrained_model_path and --max_seq_len are required (there they fail later, inside
the tokenizer); a line of neither form and an item id raw/item_info.jsonl lacks are errors that name the line (there: the previous
line's text, or a NameError / KeyError); the result is allocated once on the device and filled batch by batch (there: one torch.cat
of the whole matrix per step); one GPU only.  --adjacency (not in the reference, which lost its writer) also writes
processed/adj_t.pt, the `edge_index` of item_alignment_amd.data.build_edge_index, the second file finetune_graph.py reads.
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def build_parser():
    parser = argparse.ArgumentParser()
    a = parser.add_argument
    a("--data_dir", required=True, type=str, help="data directory: raw/item_info.jsonl and processed/entity2id.txt are read, processed/ is written")
    a("--output_dir", required=True, type=str, help="directory --config_file is looked up in")
    a("--config_file", required=True, type=str, help="model configuration (json), relative to --output_dir")
    # the reference's training flags: accepted, most of them never read
    a("--seed", default=2345, type=int, help="seed of whatever the pretrained files leave to the initialiser")
    a("--train_batch_size", default=64, type=int, help="accepted, not read")
    a("--eval_batch_size", default=64, type=int, help="texts per forward pass")
    a("--learning_rate", default=1e-3, type=float, help="accepted, not read")
    a("--start_epoch", default=0, type=int, help="accepted, not read")
    a("--num_train_epochs", default=1000, type=int, help="accepted, not read")
    a("--weight_decay", default=1e-5, type=float, help="accepted, not read")
    a("--log_steps", default=None, type=int, help="log a line every n batches")
    a("--pretrained_model_path", required=True, default=None, type=str, help="directory with vocab.txt and the RoBERTa weights")
    a("--file_state_dict", default=None, type=str, help="a RobertaModel state_dict to load over the pretrained weights")
    a("--type_vocab_size", default=2, type=int, help="accepted, not read (the configuration file decides)")
    a("--parameters_to_freeze", default=None, type=str, help="accepted, not read")
    a("--threshold", default=0.5, type=float, help="accepted, not read")
    a("--warmup_proportion", default=0.1, type=float, help="accepted, not read")
    a("--gradient_accumulation_steps", default=1, type=int, help="accepted, not read")
    a("--adam_epsilon", default=1e-8, type=float, help="accepted, not read")
    a("--fp16", action="store_true", help="kept for CLI compatibility: the HIP engine always computes in bf16 with fp32 master weights")
    a("--margin", default=1.0, type=float, help="accepted, not read")
    a("--do_lower_case", default=True, type=bool, help="lower-case the texts before the vocabulary lookup")
    a("--max_seq_len", required=True, default=None, type=int, help="tokens per text, [CLS] and [SEP] included")
    a("--max_seq_len_pv", default=None, type=int, help="only enters the position-table check")
    a("--max_position_embeddings", default=512, type=int, help="must be at least 2 * (max_seq_len + max_seq_len_pv) + 2")
    a("--max_pvs", default=20, type=int, help="accepted, not read")
    a("--cls_layers", default="1", type=str, help="accepted, not read")
    a("--cls_pool", default="cat", type=str, help="accepted, not read")
    a("--auxiliary_task", action="store_true", help="accepted, not read")
    a("--filter_sizes", default="1,2,3,5", type=str, help="accepted, not read")
    a("--num_filters", default=36, type=int, help="accepted, not read")
    # not in the reference
    a("--adjacency", action="store_true", help="also write processed/adj_t.pt (edge_index of the item / value graph)")
    return parser


def get_parser(argv=None):
    return build_parser().parse_args(argv)


def load_raw_data(args):
    """reference pred_text.py:65-93: [(id column, segmented text)] in the order of entity2id.txt"""
    from item_alignment_amd.data.datasets import _cut
    from item_alignment_amd.data.graph_files import read_entity_lines, read_item_info
    from item_alignment_amd.utils import logger
    info = read_item_info(os.path.join(args.data_dir, "raw", "item_info.jsonl"))
    logger.info(f"Finished loading item info, size: {len(info)}")
    path = os.path.join(args.data_dir, "processed", "entity2id.txt")
    data = []
    for no, (key, idx) in enumerate(read_entity_lines(path), 1):
        if key.startswith("/item/"):
            item = key[len("/item/"):]
            if item not in info:
                raise ValueError(f"{path} entry {no} ({key!r}): item id {item!r} is not in raw/item_info.jsonl")
            text = info[item]["title"]
        elif key.startswith("/value/"):
            text = key[len("/value/"):]
        else:
            raise ValueError(f"{path} entry {no}: {key!r} is neither /item/<id> nor /value/<v>")
        data.append((idx, _cut(text)))
    return data


def main(argv=None):
    args = get_parser(argv)
    if int(os.environ.get("WORLD_SIZE", "1")) > 1:
        raise SystemExit("pred_text.py runs on one GPU (WORLD_SIZE must be 1): it is one forward pass over the entity list")
    import torch
    from torch.utils.data import DataLoader
    from item_alignment_amd import train
    from item_alignment_amd.cli_common import load_config, load_tokenizer, pick_device
    from item_alignment_amd.data import RobertaDataset, build_edge_index, collate
    from item_alignment_amd.models.text import RobertaModel
    from item_alignment_amd.utils import logger

    train.seed_everything(args.seed)
    if args.fp16:
        logger.info("--fp16: the HIP engine computes in bf16 with fp32 accumulation whatever this flag says")
    msl = args.max_seq_len if args.max_seq_len_pv is None else args.max_seq_len + args.max_seq_len_pv
    assert args.max_position_embeddings >= 2 * msl + 2
    tokenizer = load_tokenizer(args)
    config = load_config(os.path.join(args.output_dir, args.config_file), max_seq_len=args.max_seq_len, ensemble=None)
    model = RobertaModel.from_pretrained(args.pretrained_model_path, config=config, ignore_mismatched_sizes=True)
    if args.file_state_dict is not None:
        model.load_state_dict(torch.load(args.file_state_dict, map_location="cpu"))
    data = load_raw_data(args)
    logger.info(f"# test samples: {len(data)}")
    if [idx for idx, _ in data] != list(range(len(data))):
        logger.warning("the id column of entity2id.txt is not 0..N-1 in file order: row k of feature_matrix.pt is LINE k of the file, "
                       "while finetune_graph.py indexes the rows by id")
    processed = os.path.join(args.data_dir, "processed")
    if args.adjacency:
        edge_index = build_edge_index(args.data_dir)
        torch.save(edge_index, os.path.join(processed, "adj_t.pt"))
        logger.info(f"adj_t.pt: {edge_index.shape[1]} directed edges")

    device = pick_device(model)
    model.to(device)
    model.eval()
    loader = DataLoader(RobertaDataset(data, tokenizer, max_seq_len=args.max_seq_len), batch_size=args.eval_batch_size, shuffle=False,
                        collate_fn=collate)
    feature_matrix = torch.empty((len(data), config.hidden_size), device=device, dtype=torch.float32)
    row = 0
    with torch.no_grad():
        for step, batch in enumerate(loader):
            input_ids, segment_ids, input_mask, position_ids = (t.to(device, non_blocking=True) if t is not None else None
                                                                for t in batch[1:])
            output = model(input_ids=input_ids, token_type_ids=segment_ids, attention_mask=input_mask, position_ids=position_ids,
                           return_pooler_output=True, padded_rows_unread=True, cls_only_read=True)
            n = input_ids.shape[0]
            feature_matrix[row:row + n] = output.pooler_output
            row += n
            if args.log_steps is not None and step % args.log_steps == 0:
                logger.info(f"[Prediction] {step} samples processed")
    torch.save(feature_matrix.cpu(), os.path.join(processed, "feature_matrix.pt"))
    logger.info("[Prediction] Finished processing")


if __name__ == "__main__":
    main()
