"""Times the TextCNN two-tower train step (forward + backward + TorchAdamW, dropout 0.1) at BASELINE config C1 (32 pairs, L = 255,
H = 1024, 36 filters of sizes 1,2,3,5, vocabulary 21128) and at the reference train.sh's 256 pairs, on one GPU through the HIP kernels
and on the host cores through the plain torch modules (the only path before the kernels existed), on the same machine.

    python tools/textcnn_bench.py [--pairs 32,256 --steps 20 --warmup 5 --cpu-steps 3 --cpu-warmup 1 --out profiles/textcnn_bench.json]

Every figure is the median of the timed steps after the warm-up steps; GPU steps are timed with events on the stream, CPU steps with
the wall clock.  The JSON holds both numbers per batch size and their ratio.
"""
import argparse
import json
import os
import sys
import time
from types import SimpleNamespace

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def config():
    return SimpleNamespace(hidden_size=1024, vocab_size=21128, max_position_embeddings=512, type_vocab_size=2, pad_token_id=0,
                           hidden_dropout_prob=0.1, layer_norm_eps=1e-12, num_labels=2, classification_method="cls", loss_type="ce",
                           loss_margin=1.0, filter_sizes="1,2,3,5", num_filters=36)


def batch(cfg, pairs, L, device, seed=1):
    g = torch.Generator().manual_seed(seed)
    ids = [torch.randint(5, cfg.vocab_size, (pairs, L), generator=g) for _ in range(2)]
    lens = torch.randint(L // 3, L + 1, (2, pairs), generator=g)
    for t, n in zip(ids, lens):
        t[torch.arange(L)[None, :] >= n[:, None]] = cfg.pad_token_id
    labels = torch.randint(0, 2, (pairs,), generator=g)
    return dict(input_ids_1=ids[0].to(device), input_ids_2=ids[1].to(device), labels=labels.to(device))


def median(v):
    return sorted(v)[len(v) // 2]


def run(device, pairs, L, steps, warmup):
    from item_alignment_amd.models import TextCNNTwoTower
    from item_alignment_amd.models import functional as Fn
    from item_alignment_amd.train import TorchAdamW
    torch.manual_seed(0)
    cfg = config()
    model = TextCNNTwoTower(cfg, {}).to(device).train()
    opt = TorchAdamW(model, 1e-3, 1e-8, 1e-5)
    b = batch(cfg, pairs, L, device)
    gpu = torch.device(device).type == "cuda"
    times, loss = [], None
    for i in range(warmup + steps):
        Fn.set_step_seed(1000 + i)
        if gpu:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
        else:
            t0 = time.perf_counter()
        opt.zero_grad()
        loss = model(**b).loss
        loss.backward()
        opt.step(1.0)
        if gpu:
            e1.record()
            torch.cuda.synchronize()
            ms = e0.elapsed_time(e1)
        else:
            ms = (time.perf_counter() - t0) * 1e3
        if i >= warmup:
            times.append(ms)
    return dict(ms_per_step=median(times), min_ms=min(times), max_ms=max(times), steps=steps, warmup=warmup, final_loss=float(loss.detach()))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", default="32,256")
    ap.add_argument("--seq-len", type=int, default=255)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--cpu-steps", type=int, default=3)
    ap.add_argument("--cpu-warmup", type=int, default=1)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "textcnn_bench.py compares one GPU with the host cores of the same machine"
    res = dict(model="TextCNNTwoTower", seq_len=a.seq_len, hidden_size=1024, filter_sizes="1,2,3,5", num_filters=36, vocab_size=21128,
               gpu=torch.cuda.get_device_name(0), cpu_threads=torch.get_num_threads(), runs=[])
    for pairs in (int(v) for v in a.pairs.split(",")):
        g = run("cuda:0", pairs, a.seq_len, a.steps, a.warmup)
        c = run("cpu", pairs, a.seq_len, a.cpu_steps, a.cpu_warmup)
        row = dict(pairs=pairs, gpu=g, cpu=c, cpu_over_gpu=c["ms_per_step"] / g["ms_per_step"])
        res["runs"].append(row)
        print(f"pairs {pairs}: GPU {g['ms_per_step']:.2f} ms/step, host cores ({res['cpu_threads']} threads) {c['ms_per_step']:.1f} ms/step, "
              f"ratio {row['cpu_over_gpu']:.1f}", flush=True)
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
