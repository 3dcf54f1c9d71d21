#!/usr/bin/env python3
"""Uniform model soup over the per-epoch checkpoints of finetune_text.py, then evaluation / prediction with the averaged weights:
the reference's model_soup_text.py (flags :33-81, soup :225-251, output names :245-249, :411).  --soups lists the epochs,
--file_state_dict is a pattern with `{}` in place of the epoch.  Parameters are averaged over the listed epochs, entries that are not
parameters come from the last listed checkpoint.  The soup is saved beside the checkpoints as pkgm_finetune-uniform_soup-epoch-<soups>.bin
(the reference's name, whatever the model family); --do_eval sweeps the thresholds on the validation file and --do_pred writes
deepAI_result_uniform_soup_threshold=<t>.jsonl, both through the harness finetune_text.py runs on (the data files are the ones that
script reads).  Every flag of finetune_text.py is accepted; training is off.
"""
import os

import torch

import finetune_text as FT
from item_alignment_amd.soup import load_soup, uniform_soup
from item_alignment_amd.utils import logger

PATH_FIELDS = ("model_name", "data_version", "interaction_type", "classification_method", "similarity_measure", "loss_type")


def soup_flags(parser):
    """what the reference's parser has and finetune_text.py's lacks or sets otherwise"""
    parser.add_argument("--soups", required=True, type=str, help="epochs whose checkpoints are averaged, comma-separated, e.g. 0,1,2")
    for action in parser._actions:
        if action.dest == "file_state_dict":
            action.required = True
            action.help = "checkpoint path pattern with {} in place of the epoch"
    parser.set_defaults(log_steps=None, max_pvs=20)


def build_parser():
    return FT.build_parser(soup_flags)


def main():
    args = build_parser().parse_args()
    pattern, args.file_state_dict = args.file_state_dict, None           # the pattern is not a checkpoint to resume from
    if "{}" not in pattern:
        raise ValueError("--file_state_dict must be a path pattern with {} in place of the epoch")
    args.do_train = False
    args.pred_tag = "uniform_soup_"

    def soup(args, model):
        epochs = args.soups.split(",")
        st = uniform_soup(model, pattern, epochs)
        load_soup(model, st, epochs, logger)
        out_dir = os.path.join(args.output_dir, "-".join(str(getattr(args, f)) for f in PATH_FIELDS))
        os.makedirs(out_dir, exist_ok=True)
        torch.save(st, os.path.join(out_dir, f"pkgm_finetune-uniform_soup-epoch-{args.soups}.bin"))
        logger.info("Finished saving uniform soup model")

    FT.main(args, before_run=soup)


if __name__ == "__main__":
    main()
