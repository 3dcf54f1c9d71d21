"""image_embedding.py without a GPU: its I/O with a stub tower injected (JSON layout, unreadable and missing images as zeros with the
counters, an existing output file returned untouched), the checkpoint key handling and both usage errors."""
import json
import logging
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import image_embedding as IE  # noqa: E402


class StubTower:
    """embed = per-image means of the three channels and the image's corner value, padded to num_features"""
    num_features = 6

    def __init__(self):
        self.batches = []

    def embed(self, images):
        assert images.dim() == 4 and images.shape[1] == 3 and images.dtype == torch.float32
        self.batches.append(images.shape[0])
        m = images.mean((2, 3))
        return torch.cat([m, images[:, :, 0, 0]], 1)


def make_data(tmp_path, n=5):
    from PIL import Image
    data, out = tmp_path / "data", tmp_path / "out"
    (data / "item_images_cropped").mkdir(parents=True)
    rs = np.random.RandomState(3)
    ids = [f"item{i}" for i in range(n)] + ["broken", "absent"]
    with open(data / "item_info.jsonl", "w", encoding="utf-8") as w:
        for i in ids:
            w.write(json.dumps({"item_id": i, "item_image_name": "ignored.jpg", "title": "标题"}, ensure_ascii=False) + "\n")
        w.write("\n")
    for i in ids[:n]:
        Image.fromarray(rs.randint(0, 256, (40, 52, 3), dtype=np.uint8)).save(data / "item_images_cropped" / f"{i}.jpg", quality=90)
    (data / "item_images_cropped" / "broken.jpg").write_bytes(b"this is no JPEG file")
    return str(data), str(out), ids


def args_for(data, out, *extra):
    return IE.parse_args(["--data_dir", data, "--output_dir", out, "--pretrained_model_path", "unused.bin", "--image_size", "32", "--batch_size", "3",
                          "--cv_model_name", "eca_nfnet_l0", *extra])


def test_json_layout_zeros_and_counters(tmp_path, caplog):
    data, out, ids = make_data(tmp_path)
    tower = StubTower()
    with caplog.at_level(logging.INFO):
        emb = IE.load_image_embedding(args_for(data, out), tower, "cpu")
    text = caplog.text
    assert list(emb) == ids                                            # the file's order
    assert emb["broken"] == [0.0] * 6 and emb["absent"] == [0.0] * 6
    assert "[CV Error] broken broken.jpg" in text and "[CV Error] absent absent.jpg" in text
    assert "Finished processing images! Total: 7, Missing: 0, Error: 2" in text
    assert "Finished loading image embedding dict! Length: 7" in text
    assert sum(tower.batches) == 5 and max(tower.batches) <= 3        # batches of --batch_size items, the unreadable ones not sent
    # the file: one JSON object item_id -> list of floats, fp32 values through tolist()
    with open(os.path.join(out, "image_embedding.json"), encoding="utf-8") as f:
        on_disk = json.load(f)
    assert on_disk == emb
    # the values are the eval transform's output through the tower
    from PIL import Image
    from item_alignment_amd.data.transforms import ImageTransform
    tf = ImageTransform(32, False)
    for i in ids[:5]:
        img = Image.open(os.path.join(data, "item_images_cropped", f"{i}.jpg")).convert("RGB")
        x = tf.apply(img, tf.draw(img.width, img.height))[None]
        want = StubTower().embed(x)[0].numpy().tolist()
        assert emb[i] == want and all(isinstance(v, float) for v in emb[i])
        assert np.float32(emb[i][0]) == emb[i][0]                      # an fp32 value, widened


def test_device_defaults_to_the_towers(tmp_path):
    """a tower without parameters (the stub): cpu; the result is the one with the device named"""
    data, out, ids = make_data(tmp_path, n=2)
    emb = IE.load_image_embedding(args_for(data, out), StubTower())
    assert list(emb) == ids and emb["item0"] != [0.0] * 6


def test_the_warning_says_why_and_a_defect_is_not_a_zero_vector(tmp_path, caplog, monkeypatch):
    data, out, ids = make_data(tmp_path, n=1)
    with caplog.at_level(logging.WARNING):
        IE.load_image_embedding(args_for(data, out), StubTower(), "cpu")
    assert "absent.jpg (FileNotFoundError" in caplog.text and "broken.jpg (UnidentifiedImageError" in caplog.text
    # an exception no damaged file raises is a defect of the code: it ends the run, and no file is written
    import item_alignment_amd.data.datasets as D

    def boom(*a, **k):
        raise RuntimeError("a defect")
    monkeypatch.setattr(D, "load_image", boom)
    out2 = str(tmp_path / "out2")
    with pytest.raises(RuntimeError, match="a defect"):
        IE.load_image_embedding(args_for(data, out2), StubTower(), "cpu")
    assert not os.path.exists(os.path.join(out2, "image_embedding.json"))


def test_existing_file_is_returned_untouched(tmp_path):
    data, out, _ = make_data(tmp_path, n=1)
    os.makedirs(out)
    path = os.path.join(out, "image_embedding.json")
    with open(path, "w", encoding="utf-8") as w:
        w.write('{"x": [1.5, 2.0]}')
    before = os.stat(path).st_mtime_ns
    tower = StubTower()
    assert IE.load_image_embedding(args_for(data, out), tower, "cpu") == {"x": [1.5, 2.0]}
    assert tower.batches == [] and os.stat(path).st_mtime_ns == before
    assert open(path, encoding="utf-8").read() == '{"x": [1.5, 2.0]}'


def test_checkpoint_keys():
    t = lambda: torch.zeros(1)
    plain = {"stem.conv1.weight": t(), "stages.0.0.conv1.gain": t(), "head.fc.weight": t(), "head.fc.bias": t()}
    assert sorted(IE.tower_state_dict(plain)) == ["stages.0.0.conv1.gain", "stem.conv1.weight"]
    pair = {"img_encoder.stem.conv1.weight": t(), "img_encoder.final_conv.bias": t(), "img_encoder.head.fc.weight": t(), "classifier.dense.weight": t(),
            "classifier.out_proj.bias": t()}
    assert sorted(IE.tower_state_dict(pair)) == ["final_conv.bias", "stem.conv1.weight"]


def test_the_tower_loads_both_checkpoint_layouts(tmp_path):
    from item_alignment_amd.models.nfnet import NormFreeNet
    net = NormFreeNet((1, 1, 1, 1), (256, 512, 512, 512), 1.0)
    sd = {k: v.clone() for k, v in net.state_dict().items()}
    for keys in (sd, {"img_encoder." + k: v for k, v in sd.items()} | {"classifier.dense.weight": torch.zeros(2, 2)}):
        other = NormFreeNet((1, 1, 1, 1), (256, 512, 512, 512), 1.0)
        missing, unexpected = other.load_state_dict(IE.tower_state_dict(keys), strict=False)
        assert not unexpected and all(k.startswith("head.") for k in missing)
        assert torch.equal(other.stem.conv1.weight, net.stem.conv1.weight) and torch.equal(other.final_conv.gain, net.final_conv.gain)


@pytest.mark.parametrize("argv,needle", [
    (["--cv_model_name", "vit_base_patch16_384", "--pretrained_model_path", "x.bin"], "embed()"),
    (["--cv_model_name", "no_such_tower", "--pretrained_model_path", "x.bin"], "no HIP tower"),
    (["--cv_model_name", "eca_nfnet_l1"], "--pretrained_model_path is required")])
def test_usage_errors(capsys, argv, needle):
    with pytest.raises(SystemExit) as e:
        IE.parse_args(["--data_dir", "d", "--output_dir", "o"] + argv)
    assert e.value.code == 2
    assert needle in capsys.readouterr().err


def test_defaults_are_the_references():
    a = IE.parse_args(["--data_dir", "d", "--output_dir", "o", "--pretrained_model_path", "x.bin"])
    assert (a.cv_model_name, a.image_size, a.batch_size, a.finetuned, a.gpu_jpeg, a.gpu_preproc, a.num_workers) == ("eca_nfnet_l1", 1000, 256, False, False,
                                                                                                                 False, 0)
