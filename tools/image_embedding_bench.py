"""Forward-only ECA-NFNet: images/s of NormFreeNet.embed against the same tower's existing forward under torch.no_grad().

    python tools/image_embedding_bench.py --out profiles/image_embedding_bench.json

Rows: eca_nfnet_l1 and eca_nfnet_l0 at 800 x 800, batch 64 (what image_embedding.py runs per batch at --image_size 800), seeded
weights and seeded normal images already on the device: the tower alone, no decode and no transform.  Arms, in one process:
  forward   net(images) under torch.no_grad(): the path evaluation and prediction use today -- every SiLU a pass of its own, every
            weight standardised on every call, every feature map allocated per call
  embed     net.embed(images): activation epilogues in the direct 3x3 kernels, SiLU + pool in one read, held weights, owned buffers
After one warm-up of each arm, --rounds (4) rounds; a round times both arms, in the order forward, embed in even rounds and embed,
forward in odd ones; one timing = --iters (3) calls between two device events.  Medians and the min / max of the rounds are reported,
and embed's output is compared with forward's on the same batch (rel-rms; both are bf16 towers, embed rounds less often).
Needs the GPU: there is no fallback.
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed(fn, iters):
    import torch
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        out = fn()
    b.record()
    torch.cuda.synchronize()
    del out
    return a.elapsed_time(b) / iters


def measure(name, size, batch, rounds, iters):
    import torch
    from item_alignment_amd.models.nfnet import create_nfnet
    torch.manual_seed(7)
    net = create_nfnet(name)
    with torch.no_grad():
        for blk in (b for st in net.stages for b in st):
            blk.conv3.gain.fill_(1.0)                  # (timm initialises it to 0: the residual branches would carry nothing)
    net = net.cuda().eval()
    images = torch.randn((batch, 3, size, size), generator=torch.Generator().manual_seed(1)).cuda()

    def forward():
        with torch.no_grad():
            return net(images)

    def embed():
        return net.embed(images)

    f, e = forward().double(), embed().double()        # warm-up of both arms (embed's builds its plan and holds the weights)
    torch.cuda.synchronize()
    diff = float((e - f).norm() / f.norm())
    ms = {"forward": [], "embed": []}
    for r in range(rounds):
        for arm in (("forward", "embed"), ("embed", "forward"))[r % 2]:
            ms[arm].append(timed(forward if arm == "forward" else embed, iters))
    row = {"tower": name, "image_size": size, "batch": batch, "rounds": rounds, "iters_per_timing": iters, "embed_vs_forward_rel_rms": diff}
    for arm, v in ms.items():
        med = statistics.median(v)
        row[arm] = {"ms_per_batch_median": med, "ms_per_batch_min_max": [min(v), max(v)], "images_per_s": batch * 1e3 / med}
    row["embed_over_forward"] = row["embed"]["images_per_s"] / row["forward"]["images_per_s"]
    row["peak_memory_gib"] = torch.cuda.max_memory_allocated() / 2 ** 30
    del net, images
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "image_embedding_bench.json"))
    ap.add_argument("--towers", default="eca_nfnet_l1,eca_nfnet_l0")
    ap.add_argument("--image_size", type=int, default=800)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--iters", type=int, default=3)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("image_embedding_bench needs the GPU")
    result = {"device": torch.cuda.get_device_name(0), "rows": []}
    for name in args.towers.split(","):
        row = measure(name, args.image_size, args.batch, args.rounds, args.iters)
        result["rows"].append(row)
        print(json.dumps(row), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps({r["tower"]: (round(r["forward"]["images_per_s"], 1), round(r["embed"]["images_per_s"], 1)) for r in result["rows"]}))


if __name__ == "__main__":
    main()
