"""pred_text.py end to end on the GPU, and the chain it exists for: a 13-entity data directory (6 items, 7 values, a small fact file)
-> processed/feature_matrix.pt + processed/adj_t.pt -> one epoch of finetune_graph.py on those two files."""
import json
import math
import os
import re
import subprocess
import sys
from types import SimpleNamespace

import pytest
import torch

from test_cli_textcnn import ROOT, WORDS, make_data

pytestmark = pytest.mark.gpu

H, MAX_SEQ_LEN = 128, 8
ASCII = [w for w in WORDS if w.isascii()]                   # one token each whatever the tokenizer does with CJK characters
ITEMS = [dict(item_id=f"i{k}", title=" ".join(ASCII[(k + j) % len(ASCII)] for j in range(1 + k)), cate_name=f"c{k % 2}",
              cate_id=str(1 + k % 2), industry_name=f"ind{k % 2}", item_image_name=f"i{k}.jpg") for k in range(6)]
VALUES = ["c0-1", "c1-2", "ind0", "红色 大号", "棉", "x y a1 b2 x y a1 b2 x", "ind1"]
# (one text longer than max_seq_len; the last line of the file has edges, as the largest id with an edge sizes the graph)
FACTS = [(0, 0, 9), (1, 1, 10), (2, 0, 9), (3, 1, 11), (5, 0, 10), (0, 0, 9)]


def _data_dir(root):
    pre = make_data(root, n_train=4, n_test=4)                          # the tiny pretrained directory (vocab.txt)
    with open(os.path.join(root, "raw", "item_info.jsonl"), "w", encoding="utf-8") as w:
        for d in ITEMS:
            w.write(json.dumps(d, ensure_ascii=False) + "\n")
    entities = [f"/item/{d['item_id']}" for d in ITEMS] + [f"/value/{v}" for v in VALUES]
    assert len(entities) == 13
    with open(os.path.join(root, "processed", "entity2id.txt"), "w", encoding="utf-8") as w:
        for k, e in enumerate(entities):
            w.write(f"{e}\t{k}\n")
    with open(os.path.join(root, "processed", "relation2id.txt"), "w", encoding="utf-8") as w:
        w.write("r0\t0\nr1\t1\n")
    with open(os.path.join(root, "processed", "train2id.txt"), "w", encoding="utf-8") as w:
        for h, r, t in FACTS:
            w.write(f"{h}\t{r}\t{t}\n")
    pairs = [(a, b, (a + b) % 2) for a in range(6) for b in range(a + 1, 6)][:12]
    for name, rows in (("item_train_train_pair.jsonl", pairs[:8]), ("item_train_valid_pair.jsonl", pairs[8:]), ("item_valid_pair.jsonl", pairs[8:])):
        with open(os.path.join(root, "raw", name), "w", encoding="utf-8") as w:
            for a, b, lab in rows:
                w.write(json.dumps({"src_item_id": f"i{a}", "tgt_item_id": f"i{b}", "item_label": str(lab)}) + "\n")
    vocab_size = len(open(os.path.join(pre, "vocab.txt"), encoding="utf-8").read().split("\n")) - 1
    cfg = dict(hidden_size=H, num_hidden_layers=2, num_attention_heads=2, intermediate_size=256, vocab_size=vocab_size,
               max_position_embeddings=64, type_vocab_size=2, hidden_dropout_prob=0.1, attention_probs_dropout_prob=0.1)
    out = os.path.join(root, "out")
    os.makedirs(out)
    json.dump(cfg, open(os.path.join(out, "roberta_tiny.json"), "w"))
    json.dump({"hidden_dropout_prob": 0.1, "num_labels": 2}, open(os.path.join(out, "gcn.json"), "w"))
    return pre, out


def _run(cmd):
    env = dict(os.environ, PYTHONPATH=ROOT)
    env.pop("WORLD_SIZE", None)
    r = subprocess.run(cmd, capture_output=True, text=True, cwd=ROOT, env=env, timeout=600)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    return r.stdout + r.stderr


def test_pred_text_writes_the_two_graph_files_and_finetune_graph_trains_on_them(gpu, tmp_path):
    import pred_text
    from item_alignment_amd.cli_common import load_config, load_tokenizer
    from item_alignment_amd.data import RobertaDataset, build_edge_index, collate
    from item_alignment_amd.models.text import RobertaModel
    root = str(tmp_path)
    pre, out = _data_dir(root)
    torch.manual_seed(7)
    config = load_config(os.path.join(out, "roberta_tiny.json"))
    model = RobertaModel(config)
    weights = os.path.join(root, "roberta_weights.bin")
    torch.save(model.state_dict(), weights)

    _run([sys.executable, os.path.join(ROOT, "pred_text.py"), "--data_dir", root, "--output_dir", out, "--config_file", "roberta_tiny.json",
          "--pretrained_model_path", pre, "--file_state_dict", weights, "--max_seq_len", str(MAX_SEQ_LEN), "--max_position_embeddings", "64",
          "--eval_batch_size", "5", "--log_steps", "1", "--fp16", "--adjacency"])

    fm = torch.load(os.path.join(root, "processed", "feature_matrix.pt"), map_location="cpu", weights_only=False)
    assert not fm.is_cuda and fm.dtype == torch.float32 and tuple(fm.shape) == (13, H) and torch.isfinite(fm).all()
    # the same weights, the same three batches (5, 5, 3), in this process
    args = SimpleNamespace(data_dir=root, pretrained_model_path=pre, do_lower_case=True)
    ds = RobertaDataset(pred_text.load_raw_data(args), load_tokenizer(args), MAX_SEQ_LEN)
    model = model.cuda().eval()
    rows = []
    with torch.no_grad():
        for lo in (0, 5, 10):
            ids, input_ids, tts, mask, pos = collate([ds[i] for i in range(lo, min(lo + 5, 13))])
            assert pos is None
            rows.append(model(input_ids=input_ids.cuda(), token_type_ids=tts.cuda(), attention_mask=mask.cuda(), return_pooler_output=True,
                              padded_rows_unread=True, cls_only_read=True).pooler_output.cpu())
    want = torch.cat(rows)
    assert float(want.abs().max()) > 0 and len({tuple(r.tolist()) for r in want[:6]}) == 6       # six different titles, 1 .. 6 tokens
    for k in range(13):
        assert torch.equal(fm[k], want[k]), k

    adj = torch.load(os.path.join(root, "processed", "adj_t.pt"), map_location="cpu", weights_only=False)
    assert adj.dtype == torch.long and torch.equal(adj, build_edge_index(root)) and adj.shape[1] > 0 and int(adj.max()) == 12

    log = _run([sys.executable, os.path.join(ROOT, "finetune_graph.py"), "--data_dir", root, "--output_dir", out, "--config_file", "gcn.json",
                "--model_name", "gcn", "--data_version", "v1", "--interaction_type", "two_tower", "--classification_method", "cls",
                "--similarity_measure", "NA", "--loss_type", "ce", "--feature_dim", str(H), "--hidden_size", "64", "--num_layers", "2",
                "--train_batch_size", "4", "--eval_batch_size", "4", "--do_train", "--num_train_epochs", "1", "--save_epochs", "1"])
    assert "graph: 13 nodes" in log, log[-2000:]
    loss = re.search(r"\[Epoch-0\] mean training loss: ([-+0-9.einfa]+)", log)
    assert loss and math.isfinite(float(loss.group(1))), log[-2000:]
    assert os.path.exists(os.path.join(out, "gcn-v1-two_tower-cls-NA-ce", "graph_epoch-0.bin"))
