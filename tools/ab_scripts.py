"""What the training scripts of one checkout compute, as one JSON, so that two checkouts can be compared entry by entry.

    python tools/ab_scripts.py run CHECKOUT --work DIR --out A.json      # run CHECKOUT's scripts, fingerprint what they wrote
    python tools/ab_scripts.py diff A.json B.json                        # the entries that differ

`run` starts bert_pretrain.py, finetune_bert.py (with one resume), coca_pretrain.py (also with --gradient_accumulation_steps 2),
finetune_text.py, finetune_image.py, finetune_multimodal.py, finetune_graph.py and pkgm_pretrain.py of CHECKOUT, each as one process,
and the data-parallel ones also as two ranks over gloo (bert_pretrain.py, finetune_bert.py, coca_pretrain.py) or as the launcher's only
rank with forced collectives (finetune_text.py: see Runs.child), on the synthetic inputs of CHECKOUT's own CLI tests: their helpers are
imported from CHECKOUT/tests, so their ROOT is CHECKOUT and every child runs CHECKOUT's code (its built library included).  Every
child has a time limit; the first non-zero exit ends the run.  The JSON holds a sha256 per tensor of every model / checkpoint file
written, a sha256 of every jsonl and csv output, and the loss / metric lines of every log with the timestamps stripped.
"""
import argparse
import hashlib
import importlib
import json
import os
import re
import subprocess
import sys

# "2026-01-01 00:00:00,000 - " of the BERT scripts' loggers, "2026/01/01 00:00:00 INFO [train.py:217]  " of the package's: the line
# number in the second moves with every edit of the file
STAMP = re.compile(r"^(\d{4}-\d\d-\d\d \d\d:\d\d:\d\d[,.]\d+ - |\d{4}/\d\d/\d\d \d\d:\d\d:\d\d (\w+) \[[\w.]+:\d+\]\s+)")
VOLATILE = re.compile(r"( - Total cost: .*$)|([-+0-9.e]+ triples/s)")          # finetune_bert.py's elapsed time, pkgm_pretrain.py's rate
KEPT = re.compile(r"loss|threshold=", re.I)


def log_lines(text, ordered, work):
    lines = [VOLATILE.sub("", STAMP.sub("", l)).rstrip().replace(work, "<work>") for l in text.splitlines() if KEPT.search(l)]
    return lines if ordered else sorted(lines)          # two ranks interleave their lines as they please


def tensor_hashes(obj, prefix, out):
    import torch
    if torch.is_tensor(obj):
        out[prefix] = hashlib.sha256(obj.detach().cpu().contiguous().reshape(-1).view(torch.uint8).numpy().tobytes()).hexdigest()
    elif isinstance(obj, dict):
        for k, v in obj.items():
            tensor_hashes(v, f"{prefix}/{k}", out)
    elif isinstance(obj, (int, float, str)):
        out[prefix] = repr(obj)


def fingerprint(work):
    """every file a script wrote under `work` -> {relative path[/tensor name]: sha256 or value}"""
    import torch
    out = {}
    for d, _, files in sorted(os.walk(work)):
        for f in sorted(files):
            path = os.path.join(d, f)
            rel = os.path.relpath(path, work)
            if f.endswith(".bin") or f == "checkpoint":
                tensor_hashes(torch.load(path, map_location="cpu", weights_only=False), rel, out)
            elif f.endswith((".jsonl", ".csv")):
                out[rel] = hashlib.sha256(open(path, "rb").read()).hexdigest()
            elif f.endswith(".log"):
                out[rel] = log_lines(open(path, encoding="utf8").read(), True, work)
    return out


class Runs:
    def __init__(self, checkout, work):
        self.root, self.work, self.logs = os.path.abspath(checkout), os.path.abspath(work), {}
        sys.path[:0] = [os.path.join(self.root, "tests"), self.root]
        self.t = {n: importlib.import_module(n) for n in ("test_bert_pretrain_cli_gpu", "test_bert_align_cli_gpu", "test_bert_dp_cli_gpu",
                                                          "test_coca_pretrain_cli_gpu", "test_coca_pretrain_dp_cli_gpu", "test_cli_gpu",
                                                          "test_cli_textcnn", "test_gcn_cli_gpu", "test_pkgm_pretrain_gpu")}
        assert all(os.path.abspath(m.__file__).startswith(self.root + os.sep) for m in self.t.values()), "helpers of another checkout"

    def dir(self, name):
        from pathlib import Path
        p = Path(self.work) / name
        p.mkdir(parents=True)
        return p

    def keep(self, name, code, log, ordered=True):
        print(f"[ab_scripts] {name}: exit {code}", flush=True)
        if code != 0:
            raise SystemExit(f"{name} failed with exit code {code}:\n{log[-4000:]}")
        self.logs[f"stdout:{name}"] = log_lines(log, ordered, self.work)

    def child(self, name, script, argv, forced_collectives=False, timeout=300):
        """one process.  forced_collectives: under the launcher as its only rank with IA_DP_FORCE_COLLECTIVES=1, the way
        tests/test_cli_gpu.py drives the data-parallel path of train.run on one GPU (cli_common.pick_device takes LOCAL_RANK as the
        device, so two ranks of finetune_text.py need two GPUs)"""
        env = dict(os.environ, PYTHONPATH=self.root, HF_HUB_OFFLINE="1", TRANSFORMERS_OFFLINE="1")
        for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT", "IA_DP_FORCE_COLLECTIVES", "IA_DP_BACKEND"):
            env.pop(k, None)
        cmd = [sys.executable]
        if forced_collectives:
            env["IA_DP_FORCE_COLLECTIVES"] = "1"
            cmd += ["-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "1", "--master-addr", "127.0.0.1", "--master-port",
                    str(self.t["test_bert_dp_cli_gpu"]._free_port())]
        r = subprocess.run(cmd + [os.path.join(self.root, script)] + [str(a) for a in argv], capture_output=True, text=True, env=env,
                           timeout=timeout, cwd=self.root)
        self.keep(name, r.returncode, r.stdout + r.stderr)

    def two_ranks(self, name, script, argv):
        """the launcher of tests/test_bert_dp_cli_gpu.py: two ranks on loopback over gloo, 300 s"""
        code, log = self.t["test_bert_dp_cli_gpu"].launch(script, [str(a) for a in argv])
        self.keep(name, code, log, ordered=False)

    def bert_pretrain(self):
        T = self.t["test_bert_pretrain_cli_gpu"]
        root = self.dir("bert_pretrain")
        model_dir, data_dir = T.write_inputs(root)
        argv = lambda out, *more: ["--data_dir", data_dir, "--model_name_or_path", model_dir, "--output_dir", root / out,
                                   "--max_seq_len", 30, "--batch_size", 4, "--num_epochs", 1, "--warmup_steps", 2, "--log_steps", 1,
                                   "--learning_rate", "1e-3", "--seed", 7] + list(more)
        r = T.run_cli([str(a) for a in argv("one", "--eval_steps", 2, "--max_steps", 4)])
        self.keep("bert_pretrain/one", r.returncode, r.stdout + r.stderr)
        self.two_ranks("bert_pretrain/two_ranks", "bert_pretrain.py", argv("two_ranks", "--eval_steps", 4))

    def finetune_bert(self):
        """the files of the `dirs` fixture of tests/test_bert_align_cli_gpu.py (a fixture cannot be imported), its train_args"""
        T = self.t["test_bert_align_cli_gpu"]
        root = self.dir("finetune_bert")
        model_dir, data_dir = root / "model", root / "data"
        os.makedirs(model_dir)
        os.makedirs(data_dir)
        (model_dir / "vocab.txt").write_text("\n".join(T.VOCAB) + "\n", encoding="utf8")
        json.dump(T.CONFIG, open(model_dir / "config.json", "w"))
        for fname, recs in (("item-align-train.json", T.pairs(24)), ("item-align-val.json", {"data": T.pairs(8, shift=3)})):
            json.dump(recs, open(data_dir / fname, "w", encoding="utf8"), ensure_ascii=False)
        dirs = (root, model_dir, data_dir)
        self.child("finetune_bert/one", "finetune_bert.py", T.train_args(dirs, "one", 6))
        self.child("finetune_bert/one_resumed", "finetune_bert.py", T.train_args(dirs, "one", 7) + ["--eval_steps", "7", "--check_steps", "7"])
        self.two_ranks("finetune_bert/two_ranks", "finetune_bert.py", T.train_args(dirs, "two_ranks", 6))

    def coca_pretrain(self):
        T, D = self.t["test_coca_pretrain_cli_gpu"], self.t["test_coca_pretrain_dp_cli_gpu"]
        paths = T.write_inputs(self.dir("coca_pretrain"))
        for name, more in (("one", ()), ("accumulated", ("--gradient_accumulation_steps", "2"))):
            log, _ = T.run_cli(paths, name, *more)          # asserts the exit code itself, 300 s
            self.keep(f"coca_pretrain/{name}", 0, log)
        code, log = D.launch(paths, "two_ranks", 29751)
        self.keep("coca_pretrain/two_ranks", code, log, ordered=False)

    def finetune_text_image_multimodal(self):
        """The inputs and arguments written out in the bodies of tests/test_cli_gpu.py (they are no helpers that could be imported; keep in
        step with them): test_finetune_text_roberta_gpu (two_tower; also with forced collectives, as test_finetune_text_under_torchrun_rccl),
        test_finetune_multimodal_roberta_image_gpu (two_tower, begin) and test_finetune_image_gpu (eca_nfnet_l0, here with --gpu_jpeg)"""
        T, make_data = self.t["test_cli_gpu"], self.t["test_cli_textcnn"].make_data
        import numpy as np
        cfg = dict(hidden_size=128, num_hidden_layers=2, num_attention_heads=2, intermediate_size=256, max_position_embeddings=64,
                   type_vocab_size=2, hidden_dropout_prob=0.1, attention_probs_dropout_prob=0.1)
        common = ["--train_batch_size", 8, "--eval_batch_size", 4, "--num_train_epochs", 1, "--learning_rate", "1e-4", "--log_steps", 1]
        text = ["--max_seq_len", 8, "--max_seq_len_pv", 12, "--max_position_embeddings", 64, "--fp16"]
        for name in ("finetune_text", "finetune_text_forced_collectives", "finetune_multimodal"):
            root = str(self.dir(name))
            pre = make_data(root, n_train=16, n_test=8)
            cfg["vocab_size"] = len(open(os.path.join(pre, "vocab.txt"), encoding="utf-8").read().split("\n")) - 1
            json.dump(cfg, open(os.path.join(root, "tiny.json"), "w"))
            os.makedirs(os.path.join(root, "out"))
            argv = ["--data_dir", root, "--output_dir", os.path.join(root, "out"), "--config_file", os.path.join(root, "tiny.json"),
                    "--data_version", "v1", "--interaction_type", "two_tower", "--classification_method", "cls", "--loss_type", "ce",
                    "--do_train", "--do_eval", "--do_pred", "--pretrained_model_path", pre] + common + text
            if name == "finetune_multimodal":
                rs, path = np.random.RandomState(3), os.path.join(root, "processed", "v1")
                for f in ("finetune_train.tsv", "finetune_test.tsv"):          # the two embedding columns of the roberta_image rows
                    rows = [l.rstrip("\n").split("\t") for l in open(os.path.join(path, f), encoding="utf-8")]
                    with open(os.path.join(path, f), "w", encoding="utf-8") as w:
                        for label, a, at, ap, b, bt, bp in rows:
                            ea, eb = (",".join(f"{float(x):.4f}" for x in rs.standard_normal(64)) for _ in range(2))
                            w.write("\t".join([label, a, at, ap, ea, b, bt, bp, eb]) + "\n")
                self.child(name, "finetune_multimodal.py", argv + ["--model_name", "roberta_image_tiny", "--ensemble", "begin", "--image_hidden_size", 64])
            else:
                argv += ["--model_name", "roberta_tiny", "--similarity_measure", "NA", "--gradient_accumulation_steps", 2]
                self.child(name, "finetune_text.py", argv, forced_collectives=name != "finetune_text")
        root = str(self.dir("finetune_image"))
        rs, items = np.random.RandomState(1), [f"i{k}" for k in range(12)]
        with open(os.path.join(root, "item_info.jsonl"), "w", encoding="utf-8") as w:
            for it in items:
                w.write(json.dumps({"item_id": it, "item_image_name": it + ".jpg"}) + "\n")
        T._images(os.path.join(root, "item_images"), [it + ".jpg" for it in items], 80)
        for fname, n in (("item_train_pair.jsonl", 8), ("item_valid_pair.jsonl", 4), ("item_test_pair.jsonl", 4)):
            with open(os.path.join(root, fname), "w", encoding="utf-8") as w:
                for _ in range(n):
                    a, b = rs.choice(items, 2, replace=False)
                    w.write(json.dumps({"src_item_id": a, "tgt_item_id": b, "item_label": str(rs.randint(2))}) + "\n")
        json.dump(dict(hidden_dropout_prob=0.1, num_labels=2), open(os.path.join(root, "img.json"), "w"))
        os.makedirs(os.path.join(root, "out"))
        self.child("finetune_image", "finetune_image.py",
                   ["--data_dir", root, "--output_dir", os.path.join(root, "out"), "--config_file", os.path.join(root, "img.json"), "--model_name",
                    "eca_nfnet_l0", "--data_version", "v1", "--do_train", "--do_eval", "--do_pred", "--train_batch_size", 4, "--eval_batch_size", 4,
                    "--num_train_epochs", 1, "--learning_rate", "1e-4", "--log_steps", 1, "--image_size", 64, "--gpu_jpeg", "--num_workers", 2])

    def finetune_graph(self):
        from item_alignment_amd.data.synthetic import SyntheticItemGraph
        g = SyntheticItemGraph(2000, 600, feature_dim=64)
        root = self.dir("finetune_graph")
        g.write(str(root / "data"))
        os.makedirs(root / "out")
        json.dump({"hidden_dropout_prob": 0.1, "num_labels": 2, "num_entities": g.num_nodes}, open(root / "out" / "gcn.json", "w"))
        log = self.t["test_gcn_cli_gpu"].run_cli(root / "data", root / "out", ["--do_train", "--do_eval", "--do_pred", "--num_train_epochs", "3", "--save_epochs",
                                                                             "1", "--log_steps", "1", "--gradient_accumulation_steps", "2"],
                                                 {"IA_GCN_PAIRWISE_LOSS": "1"})          # asserts the exit code itself, 900 s
        self.keep("finetune_graph", 0, log)

    def pkgm_pretrain(self):
        root = self.dir("pkgm_pretrain")
        self.t["test_pkgm_pretrain_gpu"].write_kg(str(root / "data"))
        self.child("pkgm_pretrain", "pkgm_pretrain.py",
                   ["--data_dir", root / "data", "--output_dir", root / "out", "--model_name", "pkgm_epoch-{}.bin", "--dim", 64, "--train_batch_size", 128,
                    "--learning_rate", "1e-2", "--num_train_epochs", 6, "--save_epochs", 3, "--log_steps", 2, "--fp16"])


def run(a):
    if os.path.exists(a.work):
        raise SystemExit(f"--work {a.work} exists already: every run starts from an empty directory")
    runs = Runs(a.checkout, a.work)
    for part in (runs.bert_pretrain, runs.finetune_bert, runs.coca_pretrain, runs.finetune_text_image_multimodal, runs.finetune_graph,
                 runs.pkgm_pretrain):
        part()
    res = dict(fingerprint(runs.work), **runs.logs)
    with open(a.out, "w") as f:
        f.write(json.dumps(res, indent=1, sort_keys=True, ensure_ascii=False) + "\n")
    print(f"[ab_scripts] {len(res)} entries -> {a.out}")


def diff(a):
    x, y = (json.load(open(p)) for p in (a.a, a.b))
    differing = sorted(k for k in set(x) | set(y) if x.get(k) != y.get(k))
    for k in differing:
        print("differs:", k, "" if k in x and k in y else "(in one file only)")
    print(f"{len(set(x) | set(y))} entries, {len(differing)} differ")
    return 1 if differing else 0


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    sub = ap.add_subparsers(dest="cmd", required=True)
    r = sub.add_parser("run")
    r.add_argument("checkout")
    r.add_argument("--work", required=True)
    r.add_argument("--out", required=True)
    d = sub.add_parser("diff")
    d.add_argument("a")
    d.add_argument("b")
    a = ap.parse_args()
    return run(a) if a.cmd == "run" else diff(a)


if __name__ == "__main__":
    sys.exit(main())
