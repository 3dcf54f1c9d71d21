"""PKGM / TransE knowledge-graph pretraining (reference pkgm_pretrain.py, run by run_pkgm_pretrain.sh) on the HIP engine.

Writes `output_dir/model_name.format(epoch)` state dicts with the keys ent_emb.weight, rel_emb.weight (and proj_mat.weight for
PKGM): the pkgm_model.bin the PKGM towers of finetune_text.py read.  The reference's flags are kept verbatim.

--do_test: after training and the final save, torchkge's link-prediction evaluation of test2id.txt (raw and filtered Hit@10, mean
rank and MRR, the reference's three lines on stdout) on the fused ranking kernel (ia_kgpt_lp_rank).  --do_eval: valid2id.txt joins the
filter, as in the reference, and is evaluated too, printed first under a `valid` line (the reference only loads it).  The filter holds
every loaded fact.  INTEGRATION.md "PKGM knowledge-graph pretraining" lists the quirks kept and the deviations.
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def get_parser():
    parser = argparse.ArgumentParser()
    parser.add_argument("--data_dir", required=True, type=str,
                        help="directory with train2id.txt, entity2id.txt, relation2id.txt (and valid2id.txt / test2id.txt for --do_eval / "
                             "--do_test)")
    parser.add_argument("--output_dir", required=True, type=str, help="The output directory where the model checkpoints will be written.")
    parser.add_argument("--model_name", default="transe_epoch-{}.bin", type=str, help="model saving name")
    parser.add_argument("--do_eval", action="store_true",
                        help="load valid2id.txt into the link-prediction filter and evaluate it after training (printed under 'valid')")
    parser.add_argument("--do_test", action="store_true", help="link-prediction evaluation of test2id.txt after training")
    parser.add_argument("--cuda_mode", default="all", help="accepted for compatibility: the whole KG always lives on the GPU")
    parser.add_argument("--train_batch_size", default=2048, type=int)
    parser.add_argument("--eval_batch_size", default=2048, type=int, help="link-prediction queries per kernel call")
    parser.add_argument("--learning_rate", default=1e-3, type=float)
    parser.add_argument("--start_epoch", default=0, type=int)
    parser.add_argument("--num_train_epochs", default=1000, type=int)
    parser.add_argument("--log_steps", default=None, type=int)
    parser.add_argument("--save_epochs", default=1000, type=int)
    parser.add_argument("--pretrained_model_path", default=None, type=str)
    parser.add_argument("--adam_epsilon", default=1e-8, type=float)
    parser.add_argument("--fp16", action="store_true", help="kept for CLI compatibility: the pretraining kernels compute in fp32")
    parser.add_argument("--weight_decay", default=1e-5, type=float)
    parser.add_argument("--warmup_proportion", default=0.2, type=float)
    parser.add_argument("--gradient_accumulation_steps", default=1, type=int)
    parser.add_argument("--dim", default=768, type=int)
    parser.add_argument("--margin", default=1.0, type=float)
    parser.add_argument("--n_neg", default=3, type=int, help="accepted; as in the reference, one negative is drawn per fact")
    parser.add_argument("--norm", default="L2", type=str, help="vector norm: L1 or L2")
    parser.add_argument("--sampling_type", default="bern", type=str, help="'bern' (Bernoulli negative sampling)")
    # not in the reference: the seed of the initialisation and of the negative sampler
    parser.add_argument("--seed", default=42, type=int)
    return parser


def _has_facts(path):
    with open(path, "r", encoding="utf-8") as f:
        return any(line.strip() for line in f)


def check_args(args):
    if (args.do_eval or args.do_test) and args.eval_batch_size <= 0:
        raise SystemExit(f"--eval_batch_size {args.eval_batch_size}: the link-prediction evaluation needs a positive batch size")
    for flag, on, fname in (("--do_eval", args.do_eval, "valid2id.txt"), ("--do_test", args.do_test, "test2id.txt")):
        if not on:
            continue
        path = os.path.join(args.data_dir, fname)
        if not os.path.isfile(path):
            raise SystemExit(f"{flag}: {path} does not exist (the link-prediction evaluation reads its facts from it)")
        if not _has_facts(path):
            raise SystemExit(f"{flag}: {path} holds no facts -- data_prepare.py's default proportions write an empty valid2id.txt / "
                             "test2id.txt; split some facts off train2id.txt first or drop the flag")
    if args.norm not in ("L1", "L2"):
        raise SystemExit(f"--norm {args.norm}: only L1 and L2 are supported (the torus dissimilarities are not built)")
    if args.sampling_type != "bern":
        raise SystemExit(f"--sampling_type {args.sampling_type}: only 'bern' is supported")
    if "transe" not in args.model_name and "pkgm" not in args.model_name:
        raise SystemExit(f"Unsuported model name: {args.model_name}")


def main(argv=None):
    args = get_parser().parse_args(argv)
    check_args(args)
    import torch
    from item_alignment_amd.models import kg_pretrain as K
    from item_alignment_amd.utils import logger

    try:
        kg, kg_valid, kg_test, filters = K.load_ccks_splits(args.data_dir, args.do_eval, args.do_test)
    except ValueError as e:
        raise SystemExit(str(e))
    if not torch.cuda.is_available():
        raise SystemExit("pkgm_pretrain.py runs on the GPU (HIP kernels, no CPU path)")
    if args.fp16:
        logger.info("--fp16: the pretraining kernels compute in fp32 (tables, projection and gradients); the flag changes nothing")
    logger.info(f"finished loading data: {len(kg)} facts, {kg.n_ent} entities, {kg.n_rel} relations")
    torch.manual_seed(args.seed)
    cls = K.TransEPretrainModel if "transe" in args.model_name else K.PKGMPretrainModel
    model = cls(args.dim, kg.n_ent, kg.n_rel, dissimilarity_type=args.norm)
    if args.pretrained_model_path is not None:
        model.load_state_dict(torch.load(args.pretrained_model_path, map_location="cpu"))
    model = model.cuda()
    optimizer = K.CoupledAdam(model.tables(), lr=args.learning_rate, weight_decay=args.weight_decay, eps=args.adam_epsilon)
    total, warmup = K.schedule_steps(len(kg), args.train_batch_size, args.gradient_accumulation_steps, args.num_train_epochs,
                                     args.start_epoch, args.warmup_proportion)
    scheduler = torch.optim.lr_scheduler.LambdaLR(optimizer, K.linear_schedule_lambda(warmup, total))
    os.makedirs(args.output_dir, exist_ok=True)
    K.train(model, kg, optimizer, scheduler, n_epochs=args.num_train_epochs, batch_size=args.train_batch_size, margin=args.margin,
            save_path=os.path.join(args.output_dir, args.model_name), start_epoch=args.start_epoch, save_epochs=args.save_epochs,
            log_steps=args.log_steps, grad_accum=args.gradient_accumulation_steps, seed=args.seed, logger=logger)
    # link prediction on the trained tables, after the final save (the reference evaluates only the test split)
    for name, split in (("valid", kg_valid), ("test", kg_test)):
        if split is None:
            continue
        evaluator = K.LinkPredictionEvaluator(model, split, filters)
        evaluator.evaluate(args.eval_batch_size)
        if name == "valid":
            print("valid", flush=True)
        evaluator.print_results()


if __name__ == "__main__":
    main()
