#!/usr/bin/env python
"""Cost of the LAMB step against the AdamW launch, on the parameter arena of the headline model (roberta_large + ViT-B/16).

Three variants on the SAME five buffers in one process: `ia_adamw_flat`, `ia_lamb_flat` without clipping and with clipping (the C entry
points themselves: no transposed-shadow refresh, no Python around them but the call).  Each round times `--iters` back-to-back launches
of every variant between two device events; the rounds alternate the order of the variants (abc, cba, ...) so that none of them always
runs first or behind the same neighbour.  Reported: the median and the range over the rounds, the ratios of the medians, and what the
byte model of DESIGN.md ("LAMB") predicts for them: 42 / 30 = 1.4 and 46 / 30 = 1.53.

    python tools/lamb_bench.py --out profiles/lamb_bench.json

Needs the GPU; there is no fallback.  To see the individual kernels, run it under `rocprofv3 --kernel-trace --stats -- python
tools/lamb_bench.py --rounds 2 --out /dev/null` in a run of its own (the kernels are lamb_gsq_kernel, lamb_scale_kernel,
lamb_moments_kernel, lamb_ratio_kernel, lamb_apply_kernel and adamw_kernel)."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

BYTES = {"adamw": 30, "lamb": 42, "lamb_clipped": 46}      # per parameter: DESIGN.md "LAMB"


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--out", required=True)
    ap.add_argument("--rounds", type=int, default=6)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--tiny", action="store_true", help="a two-layer model: for trying the tool out, not for numbers")
    args = ap.parse_args(argv)
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("lamb_bench.py measures on the GPU; none is visible")
    from bench import build_model, roberta_large_config
    from item_alignment_amd import _lib
    from item_alignment_amd._lib import check, stream_ptr
    cfg = roberta_large_config(**(dict(num_hidden_layers=2) if args.tiny else {}))
    model = build_model(cfg).cuda()
    arena = model.param_arena
    lib = _lib.load()
    torch.manual_seed(0)
    arena.grad.normal_(0.0, 1e-2)
    arena.lamb_step(1e-6)                                   # builds the tensor table and the workspace
    tables = arena._lamb
    n_params = sum(p.numel() for p in arena.params if p.requires_grad)
    step = [arena.step_count]
    lr, b1, b2, eps, wd = 1e-6, 0.9, 0.999, 1e-6, 0.01      # a learning rate that leaves the weights where they are over a few hundred steps

    def adamw():
        check(lib.ia_adamw_flat(arena.master.data_ptr(), arena.grad.data_ptr(), arena.exp_avg.data_ptr(), arena.exp_avg_sq.data_ptr(),
                                arena.shadow.data_ptr(), arena.chunk_table.data_ptr(), arena.n_chunks, lr, b1, b2, eps, wd, step[0], 1.0,
                                stream_ptr()), "ia_adamw_flat")

    variants = {"adamw": adamw,
                "lamb": lambda: tables.step(arena, lr, b1, b2, eps, wd, step[0], 1.0, 0.0),
                "lamb_clipped": lambda: tables.step(arena, lr, b1, b2, eps, wd, step[0], 1.0, 1.0)}

    def timed(fn):
        start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        for _ in range(args.iters):
            step[0] += 1
            fn()
        end.record()
        end.synchronize()
        return start.elapsed_time(end) / args.iters         # ms per call

    for fn in variants.values():                             # warm-up: code objects loaded, clocks up
        timed(fn)
    ms = {k: [] for k in variants}
    for r in range(args.rounds):
        order = list(variants) if r % 2 == 0 else list(variants)[::-1]
        for k in order:
            ms[k].append(timed(variants[k]))
    assert torch.isfinite(arena.master).all(), "the weights left the finite range during the measurement"
    med = {k: statistics.median(v) for k, v in ms.items()}
    result = {
        "tool": "tools/lamb_bench.py", "device": torch.cuda.get_device_name(0), "model": "tiny" if args.tiny else "roberta_large + vit_base_patch16_384",
        "parameters": n_params, "arena_elements": arena.numel, "chunks": tables.n_chunks, "tensors": tables.n_tensors,
        "rounds": args.rounds, "iters_per_round": args.iters, "timing": "device events around iters back-to-back calls; order alternates per round",
        "ms_per_call": {k: {"median": med[k], "min": min(v), "max": max(v), "rounds": v} for k, v in ms.items()},
        "bytes_per_parameter_model": BYTES,
        "achieved_TB_per_s_by_the_byte_model": {k: BYTES[k] * n_params / (med[k] * 1e-3) / 1e12 for k in ms},
        "ratio_to_adamw": {k: {"measured": med[k] / med["adamw"], "byte_model": BYTES[k] / BYTES["adamw"]} for k in ("lamb", "lamb_clipped")},
    }
    out_dir = os.path.dirname(os.path.abspath(args.out))
    os.makedirs(out_dir, exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps({k: result[k] for k in ("parameters", "ratio_to_adamw", "achieved_TB_per_s_by_the_byte_model")}))
    return 0


if __name__ == "__main__":
    sys.exit(main())
