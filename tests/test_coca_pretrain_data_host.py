"""MultimodalDataset + collate_coca (the data path of CoCa pre-training) against tests/golden/coca/collate_coca.json, which holds the
records and batch tuples the REFERENCE's own classes produced for the same rows (tools/gen_golden_coca_collate.py): every record key
and value and every tuple slot exactly.  The image files the rows name are written here with PIL, except the ones the fixture lists as
missing: those items must be dropped by the collate."""
import json
import os

import pytest
import torch

from fake_tokenizer import FakeBertTokenizer
from test_collate_golden import same, untensor

GOLDEN = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "coca", "collate_coca.json"), encoding="utf-8"))
CASES = {c["name"]: c for c in GOLDEN["cases"]}


def test_the_three_settings_are_there():
    assert sorted(CASES) == ["pvs_only", "title_only", "title_pvs_one_image_missing"]
    assert [len(c["missing_image"]) for c in GOLDEN["cases"]] == [0, 0, 1]


@pytest.mark.parametrize("name", sorted(CASES))
def test_records_and_batch_match_the_reference(name, tmp_path):
    from PIL import Image

    import item_alignment_amd.data.datasets as D
    case = CASES[name]
    rows = []
    for i, (item_id, title, pvs, file_name) in enumerate(case["rows"]):
        path = str(tmp_path / file_name)
        if i not in case["missing_image"]:
            Image.new("RGB", (20 + i, 24), (10 * i, 128, 255 - 10 * i)).save(path)
        rows.append((item_id, title, pvs, path))
    ds = D.MultimodalDataset(rows, text_tokenizer=FakeBertTokenizer(), **case["kw"])
    assert len(ds) == len(rows)
    recs = [ds[i] for i in range(len(ds))]
    want = untensor(case["records"])
    for i, (got, w) in enumerate(zip(recs, want)):
        assert ("image" in got) == (i not in case["missing_image"])
        if "image" in got:
            assert tuple(got["image"].shape) == (3, 16, 16) and got["image"].dtype == torch.float32
        same({k: v for k, v in got.items() if k != "image"}, {k: v for k, v in w.items() if k != "image"}, f"{name}.records[{i}]")
        assert got["position_ids"] == list(range(len(got["input_ids"])))
    # the batch of the loaded images: the missing item is gone, the order is kept
    ids, input_ids, mask, types, pos, images = D.collate_coca(recs)
    kept = [i for i in range(len(rows)) if i not in case["missing_image"]]
    assert ids == [rows[i][0] for i in kept] and tuple(images.shape) == (len(kept), 3, 16, 16)
    assert torch.equal(images, torch.stack([recs[i]["image"] for i in kept]))
    # and with the fixture's hand-made image tensors in their place, the reference's tuple exactly
    for got, w in zip(recs, want):
        got.pop("image", None)
        if "image" in w:
            got["image"] = w["image"]
    batch = D.collate_coca(recs)
    same(list(batch), untensor(case["batch"]), name + ".batch")
    assert len(batch[0]) == len(rows) - len(case["missing_image"])


def test_reference_constructor_argument_order_is_kept():
    import inspect

    import item_alignment_amd.data.datasets as D
    got = list(inspect.signature(D.MultimodalDataset.__init__).parameters)[1:]
    assert got[:8] == ["data", "image_size", "is_training", "text_tokenizer", "max_seq_len", "max_seq_len_pv", "hflip", "color_jitter"]


def test_the_new_names_import_from_every_path():
    import item_alignment_amd
    import item_alignment_amd.data as PD
    import item_alignment_amd.models as PM
    import src.data as SD
    import src.models as SM
    assert SD.MultimodalDataset is PD.MultimodalDataset and SD.collate_coca is PD.collate_coca
    assert SM.CoCaForPretraining is PM.CoCaForPretraining
    assert item_alignment_amd.models.CoCaForPretraining.__name__ == "CoCaForPretraining"
    from item_alignment_amd.models.functional import ContrastiveLossFn  # noqa: F401
    from item_alignment_amd.models.bert_pretrain import TiedCaptionHeadFn  # noqa: F401
    from item_alignment_amd import ops
    assert callable(ops.contrastive_fwd) and callable(ops.contrastive_bwd)
