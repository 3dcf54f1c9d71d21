"""Writes tests/golden/pred_text/ from the reference's own code (data only; nothing of the reference's text is copied):

    python tools/gen_golden_pred_text.py <reference checkout>

pooler.npz     the reference's RobertaModel (src/models/text.py:1084-1266) in fp32 on the CPU: 2 layers, H = 128, 2 heads, I = 512,
               vocabulary 96, 64 positions; seeded weights that are exact in bf16, stored as their 16-bit patterns (`w_<key>`);
               13 sequences padded to 24 with the valid lengths of LENGTHS; input_ids, the two masks, pooler_output and
               last_hidden_state[:, 0].
collate.json   the reference's RobertaDataset + collate (src/data/data.py:992-1033, :243-259) on 13 (idx, text) rows through
               tests/fake_tokenizer.py, under the module stubs of oracle/gen_collates.py (as tools/gen_golden_coca_collate.py).
parser.json    (flag, type, default, required) of every flag of the reference's pred_text.py, model_soup_text.py and model_ensemble.py.
ensemble/      a six-pair, three-member data directory (raw/item_info.jsonl, output/<member>/<input file>, members.json) and, under
               expected/, the file the reference's model_ensemble.py writes for {threshold, f1} x {without, with the category split};
               the module's three member lists and its category lists are set from members.json before main() is called.
"""
import argparse
import importlib.util
import json
import os
import shutil
import sys
import tempfile

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden", "pred_text")
LENGTHS = (2, 3, 4, 5, 6, 8, 10, 12, 15, 18, 20, 22, 24)
L = 24
MODEL = dict(hidden_size=128, num_hidden_layers=2, num_attention_heads=2, intermediate_size=512, vocab_size=96, max_position_embeddings=64,
             type_vocab_size=2, pad_token_id=0, hidden_dropout_prob=0.1, attention_probs_dropout_prob=0.1, layer_norm_eps=1e-12)
INPUT_FILE = "deepAI_result_threshold=0.4.jsonl"


def load_script(reference, name):
    spec = importlib.util.spec_from_file_location("reference_" + name, os.path.join(reference, name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def pooler(M, reference_config):
    rs = np.random.RandomState(1903)
    cfg = reference_config(**MODEL)
    model = M.RobertaModel(cfg).eval()
    sd = {}
    for key, val in model.state_dict().items():
        if not val.is_floating_point():
            continue
        w = rs.standard_normal(tuple(val.shape)).astype(np.float32) * 0.05
        if "LayerNorm.weight" in key:
            w += 1.0
        sd[key] = torch.from_numpy(w).to(torch.bfloat16)                 # what both sides compute with is exact in bf16
    missing, unexpected = model.load_state_dict({k: v.float() for k, v in sd.items()}, strict=False)
    assert not unexpected and all("position_ids" in k for k in missing), (missing, unexpected)
    B = len(LENGTHS)
    ids = np.zeros((B, L), np.int64)
    mask = np.zeros((B, L), np.int64)
    tts = np.zeros((B, L), np.int64)
    for b, n in enumerate(LENGTHS):
        ids[b, :n] = rs.randint(5, MODEL["vocab_size"], size=n)
        ids[b, 0] = 2
        mask[b, :n] = 1
        tts[b, n // 2:n] = 1
    with torch.no_grad():
        out = model(torch.from_numpy(ids), attention_mask=torch.from_numpy(mask), token_type_ids=torch.from_numpy(tts))
    arrays = {"w_" + k: v.view(torch.int16).numpy().view(np.uint16) for k, v in sd.items()}
    arrays.update(input_ids=ids, attention_mask=mask, token_type_ids=tts, pooler_output=out.pooler_output.numpy(),
                  cls_hidden=out.last_hidden_state[:, 0].numpy(),
                  meta=np.frombuffer(json.dumps(dict(config=MODEL, lengths=LENGTHS, transformers=__import__("transformers").__version__)).encode(),
                                     dtype=np.uint8))
    path = os.path.join(OUT, "pooler.npz")
    np.savez_compressed(path, **arrays)
    print("wrote", path, os.path.getsize(path), "bytes")


def collate_case(G):
    rs = np.random.RandomState(29)
    tk = G.FakeBertTokenizer()
    words = [n - 2 for n in LENGTHS[:-1]] + [30]                        # the last text is cut to fit: 22 words + [CLS] + [SEP]
    rows = [[7 * k + 1, " ".join(rs.choice(G.WORDS, size=n))] for k, n in enumerate(words)]
    ds = G.D.RobertaDataset([tuple(r) for r in rows], tk, L)
    recs = [ds[i] for i in range(len(ds))]
    assert [sum(r["attention_mask"]) for r in recs] == list(LENGTHS)
    out = {"max_seq_len": L, "rows": rows, "records": G.jsonable(recs), "batch": G.jsonable(G.D.collate(recs))}
    path = os.path.join(OUT, "collate.json")
    with open(path, "w", encoding="utf8") as f:
        json.dump(out, f, ensure_ascii=False, sort_keys=True)
    print("wrote", path, os.path.getsize(path), "bytes")


def parsers(reference):
    seen = {}

    class Captured(Exception):
        pass

    def capture(self, *a, **k):
        seen["parser"] = self
        raise Captured

    out = {}
    orig = argparse.ArgumentParser.parse_args
    argparse.ArgumentParser.parse_args = capture
    try:
        for name in ("pred_text", "model_soup_text", "model_ensemble"):
            mod = load_script(reference, name)
            try:
                mod.get_parser()
            except Captured:
                pass
            flags = []
            for act in seen.pop("parser")._actions:
                if act.dest == "help":
                    continue
                flags.append({"flag": act.option_strings[0], "type": None if act.type is None else act.type.__name__, "default": act.default,
                              "required": bool(act.required), "takes_value": act.nargs != 0})
            out[name] = flags
    finally:
        argparse.ArgumentParser.parse_args = orig
    path = os.path.join(OUT, "parser.json")
    with open(path, "w", encoding="utf8") as f:
        json.dump(out, f, ensure_ascii=False, sort_keys=True, indent=1)
    print("wrote", path, {k: len(v) for k, v in out.items()})


def ensemble(reference):
    rs = np.random.RandomState(5)
    root = os.path.join(OUT, "ensemble")
    if os.path.isdir(root):
        shutil.rmtree(root)
    os.makedirs(os.path.join(root, "raw"))
    cates = ["手机", "茶壶", "衬衫", "c3"]
    items = {f"i{k}": cates[k % 4] for k in range(8)}
    with open(os.path.join(root, "raw", "item_info.jsonl"), "w", encoding="utf-8") as w:
        for k, c in items.items():
            w.write(json.dumps({"item_id": k, "cate_name": c, "title": "t " + k}, ensure_ascii=False) + "\n")
    pairs = [("i0", "i4"), ("i1", "i5"), ("i0", "i3"), ("i2", "i6"), ("i3", "i7"), ("i4", "i1")]
    members = {"members": [["m_a", 0.3, 0.861], ["m_b", 0.4, 0.7777], ["m_c", 0.6, 0.851]],
               "members_in_train": [["m_a", 0.3, 0.861], ["m_b", 0.5, 0.7777], ["m_c", 0.6, 0.851]],
               "members_not_in_train": [["m_a", 0.4, 0.861], ["m_c", 0.5, 0.851]],
               "unseen_categories": ["茶壶", "衬衫"]}
    json.dump(members, open(os.path.join(root, "members.json"), "w", encoding="utf-8"), ensure_ascii=False, indent=1)
    for m, (name, _, _) in enumerate(members["members"]):
        os.makedirs(os.path.join(root, "output", name))
        order = list(range(len(pairs)))
        if m == 1:
            order = order[::-1]                                          # another order: the first member's decides
        if m == 2:
            order = [p for p in order if p != 3]                        # a member that lacks a pair
        with open(os.path.join(root, "output", name, INPUT_FILE), "w", encoding="utf-8") as w:
            for p in order:
                prob = round(float(rs.uniform(0.05, 0.95)), 4)
                emb = f"[{prob}]" if m != 1 else f"[{prob},{round(1 - prob, 4)}]"
                w.write(json.dumps({"src_item_id": pairs[p][0], "src_item_emb": f"[{round(1 - prob, 4)}]", "tgt_item_id": pairs[p][1],
                                    "tgt_item_emb": emb, "threshold": 0.4}) + "\n")
    mod = load_script(reference, "model_ensemble")
    as_tuples = lambda rows: [tuple(r) for r in rows]
    mod.models_and_thresholds = as_tuples(members["members"])
    mod.models_and_thresholds_in = as_tuples(members["members_in_train"])
    mod.models_and_thresholds_not_in = as_tuples(members["members_not_in_train"])
    mod.ONLY_TEST_CATES = list(members["unseen_categories"])
    mod.ONLY_VALID_CATES = list(members["unseen_categories"])
    os.makedirs(os.path.join(root, "expected"))
    argv = sys.argv
    for strategy in ("threshold", "f1"):
        for split in (False, True):
            with tempfile.TemporaryDirectory() as tmp:
                work = os.path.join(tmp, "data")
                shutil.copytree(root, work)
                sys.argv = ["model_ensemble.py", "--data_dir", work, "--ensemble_strategy", strategy, "--input_file", INPUT_FILE] + \
                           (["--split_by_valid_or_test"] if split else [])
                try:
                    mod.main()
                finally:
                    sys.argv = argv
                shutil.copy(os.path.join(work, "output", "ensemble", "deepAI_result.jsonl"),
                            os.path.join(root, "expected", f"{strategy}_{'split' if split else 'all'}.jsonl"))
    print("wrote", root, sorted(os.listdir(os.path.join(root, "expected"))))


def main(reference):
    sys.path.insert(0, ROOT)
    from oracle import gen_collates as G
    if not os.path.realpath(G.D.__file__).startswith(os.path.realpath(reference)):
        raise SystemExit(f"oracle/gen_collates.py imported the reference from {G.D.__file__}, not from {reference}")
    from oracle.ref_harness import load_reference, reference_config
    M = load_reference()
    os.makedirs(OUT, exist_ok=True)
    pooler(M, reference_config)
    collate_case(G)
    parsers(reference)
    ensemble(reference)


if __name__ == "__main__":
    if len(sys.argv) != 2:
        raise SystemExit(__doc__)
    main(sys.argv[1])
