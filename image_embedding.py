#!/usr/bin/env python3
"""The image embedding the roberta_image_* models read for every item: the reference's `data_prepare.py --with_image`
(load_image_embedding, data_prepare.py:275-364) on the HIP engine.  Every image $DATA_DIR/item_images_cropped/{item_id}.jpg of the
items in $DATA_DIR/item_info.jsonl goes through the eval transform and an ECA-NFNet tower's forward-only path (NormFreeNet.embed);
the pooled features are written to $OUTPUT_DIR/image_embedding.json, one JSON object item_id -> list of floats.  The reference loads
that file when it exists (:276-279), so running this script first lets the rest of its ETL run with no timm and no GPU.

Kept from the reference: the cv flags and their defaults, the paths, the transform, zeros + a warning for an image that cannot be
opened, the counters and the closing log lines, and "an existing file is loaded and returned untouched".  Not kept: with --finetuned
the reference sends the last partial batch through the classifier (:350-352, 2 logits instead of features) -- here
every item gets features.  Nothing is downloaded: the weights come from --pretrained_model_path, a tower state_dict with timm's key
names or a finetune_image.py checkpoint (its `img_encoder.` keys are taken, head / classifier keys are ignored)."""
import argparse
import json
import os

import numpy as np
import torch
from torch.utils.data import DataLoader, Dataset

from item_alignment_amd.utils import logger

HEAD_PREFIXES = ("head.", "classifier.")


def get_parser():
    p = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    a = p.add_argument
    a("--data_dir", required=True, type=str, help="模型训练数据地址")
    a("--output_dir", required=True, type=str, help="where image_embedding.json is written")
    a("--cv_model_name", default="eca_nfnet_l1", type=str, help="cv pretrained model name")
    a("--finetuned", action="store_true", help="reference flag, kept for parity: no effect here (both checkpoint layouts load with or without it)")
    a("--pretrained_model_path", default=None, type=str, help="tower state_dict (timm key names) or a finetune_image.py checkpoint")
    a("--image_size", default=1000, type=int, help="raw image size, default: 1000*1000")
    a("--batch_size", default=256, type=int, help="cv model prediction batch size")
    a("--num_workers", default=0, type=int, help="DataLoader worker processes for the decode")
    a("--gpu_preproc", action="store_true", help="decode on the host, resize / crop / normalise on the GPU (bit-identical to the Pillow path)")
    a("--gpu_jpeg", action="store_true", help="decode baseline JPEG files on the GPU as well (implies --gpu_preproc)")
    return p


def parse_args(argv=None):
    from item_alignment_amd.models.image import check_image_encoder_name
    from item_alignment_amd.models.nfnet import NFNET_CONFIGS
    p = get_parser()
    args = p.parse_args(argv)
    check_image_encoder_name(p, args.cv_model_name)
    if args.cv_model_name not in NFNET_CONFIGS:
        p.error(f"--cv_model_name {args.cv_model_name!r}: only the ECA-NFNet towers ({', '.join(sorted(NFNET_CONFIGS))}) have a forward-only "
                "embed() path yet")
    if not args.pretrained_model_path:
        p.error("--pretrained_model_path is required: nothing is downloaded here, and random weights make no embedding")
    return args


def tower_state_dict(sd):
    """the tower's own keys out of a checkpoint: the `img_encoder.`-prefixed ones of a finetune_image.py checkpoint (everything else in
    it is the pair classifier), or all of a plain tower state_dict; the tower's head / classifier keys are dropped either way"""
    if any(k.startswith("img_encoder.") for k in sd):
        sd = {k[len("img_encoder."):]: v for k, v in sd.items() if k.startswith("img_encoder.")}
    return {k: v for k, v in sd.items() if not k.startswith(HEAD_PREFIXES)}


def load_tower(args, device):
    from item_alignment_amd.models.image import create_model
    tower = create_model(args.cv_model_name, pretrained=False, img_size=args.image_size)
    missing, unexpected = tower.load_state_dict(tower_state_dict(torch.load(args.pretrained_model_path, map_location="cpu")), strict=False)
    missing = [k for k in missing if not k.startswith(HEAD_PREFIXES)]
    if missing or unexpected:
        raise SystemExit(f"{args.pretrained_model_path} is no {args.cv_model_name} state_dict: missing {missing[:5]}, unexpected {list(unexpected)[:5]}")
    return tower.to(device).eval()


class _Items(Dataset):
    """(item_id, loaded image or None, why not) per line of item_info.jsonl; the load is what the DataLoader's workers spread out.
    Only what a missing, unreadable or damaged file raises (OSError, which Pillow's UnidentifiedImageError is; ValueError and
    SyntaxError from its decoders) makes a zero vector: any other exception is a defect of this code and ends the run."""

    def __init__(self, ids, image_dir, size, raw, jpeg):
        self.ids, self.image_dir, self.size, self.raw, self.jpeg = ids, image_dir, size, raw or jpeg, jpeg
        self.transform = None

    def __len__(self):
        return len(self.ids)

    def __getitem__(self, i):
        from item_alignment_amd.data.datasets import load_image
        from item_alignment_amd.data.transforms import ImageTransform
        if self.transform is None:
            self.transform = ImageTransform(self.size, False)                   # = create_transform(input_size, is_training=False), :293
        item_id = self.ids[i]
        try:
            return item_id, load_image(os.path.join(self.image_dir, f"{item_id}.jpg"), self.transform, raw=self.raw, jpeg=self.jpeg), None
        except (OSError, ValueError, SyntaxError) as e:
            return item_id, None, f"{type(e).__name__}: {e}"


def read_item_ids(data_dir):
    ids = []
    with open(os.path.join(data_dir, "item_info.jsonl"), "r", encoding="utf-8") as r:
        for line in r:
            if line.strip():
                ids.append(json.loads(line.strip())["item_id"])
    return ids


def load_image_embedding(args, tower=None, device=None):
    """reference data_prepare.py:275-364.  tower: anything with `num_features` and `embed(images [B, 3, S, S]) -> [B, num_features]`
    (None: built from the flags on the GPU).  device: where the images go (None with a tower: the device of its parameters, cpu for
    a tower without any)."""
    file_path = os.path.join(args.output_dir, "image_embedding.json")
    if os.path.isfile(file_path):
        with open(file_path, "r", encoding="utf-8") as f:
            img_emb_dict = json.load(f)
        logger.info(f"Finished loading image embedding dict! Length: {len(img_emb_dict)}")
        return img_emb_dict
    if tower is None:
        if not torch.cuda.is_available():
            raise SystemExit("image_embedding.py runs on the MI355X HIP engine only (no CPU path); no GPU is visible")
        device = torch.device("cuda", int(os.environ.get("LOCAL_RANK", "0")))
        torch.cuda.set_device(device)
        tower = load_tower(args, device)
    elif device is None:
        device = next((p.device for p in getattr(tower, "parameters", lambda: iter(()))()), "cpu")
    device = torch.device(device)
    raw = bool(args.gpu_preproc or args.gpu_jpeg)
    pipe = None
    if raw:
        from item_alignment_amd.data.gpu_preproc import GpuImagePipeline
        pipe = GpuImagePipeline(args.image_size, device)
    ids = read_item_ids(args.data_dir)
    data = _Items(ids, os.path.join(args.data_dir, "item_images_cropped"), args.image_size, raw, bool(args.gpu_jpeg))
    nw = int(args.num_workers or 0)
    kw = dict(multiprocessing_context="forkserver") if nw > 0 else {}           # never fork() a process that owns HIP streams
    loader = DataLoader(data, batch_size=args.batch_size, shuffle=False, collate_fn=list, num_workers=nw, **kw)
    img_emb_missing = np.zeros(tower.num_features, dtype=np.float32).tolist()
    img_emb_dict = {}
    ct = ct_missing = ct_error = 0

    def failed(item_id, why):
        nonlocal ct_error
        img_emb_dict[item_id] = img_emb_missing
        logger.warning(f"[CV Error] {item_id} {item_id}.jpg ({why})")
        ct_error += 1

    for batch in loader:
        for item_id, _, _ in batch:
            img_emb_dict[item_id] = None                                         # keeps the file's order of items
        if pipe is not None:
            items = pipe.decode([im for _, im, _ in batch])                       # --gpu_jpeg: None where neither the GPU nor Pillow decodes it
            batch = [(item_id, im, why or "no decoder took the file") for (item_id, _, why), im in zip(batch, items)]
        good = [(item_id, im) for item_id, im, _ in batch if im is not None]
        for item_id, im, why in batch:
            if im is None:
                failed(item_id, why)
        if good:
            images = pipe.process([im for _, im in good]) if pipe is not None else torch.stack([im for _, im in good]).to(device)
            with torch.no_grad():
                output = tower.embed(images)
            for (item_id, _), img_emb in zip(good, output.float().cpu().numpy()):
                img_emb_dict[item_id] = img_emb.tolist()
        for _ in batch:
            if ct % 10000 == 0:
                logger.info(f"{ct} images processed")
            ct += 1
    logger.info(f"Finished processing images! Total: {ct}, Missing: {ct_missing}, Error: {ct_error}")
    os.makedirs(args.output_dir, exist_ok=True)
    with open(file_path, "w", encoding="utf-8") as w:
        json.dump(img_emb_dict, w, ensure_ascii=False)
    logger.info(f"Finished loading image embedding dict! Length: {len(img_emb_dict)}")
    return img_emb_dict


def main(argv=None):
    load_image_embedding(parse_args(argv))


if __name__ == "__main__":
    main()
