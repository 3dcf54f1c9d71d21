"""Times the causal multi-query attention kernels (ia_attn_fwd_causal_x / ia_attn_bwd_causal_x) forward + backward at the CoCa decoder's
own shape -- B = 16 sequences, Lk = 255 tokens, fold = 16 folded heads (Lq = 4080 query rows), nh = 1 -- next to ia_attn_fwd_x /
ia_attn_bwd_x at the same shape without a mask, in the same process on the same GPU.  The causal pair does about half the arithmetic.

    python tools/causal_attn_bench.py [--B 16 --Lk 255 --fold 16 --steps 50 --warmup 10 --out profiles/causal_attn_bench.json]

Every figure is the median of the timed calls after the warm-up calls, timed with events on the stream.  The JSON holds forward,
backward and their sum for both pairs, and the ratio causal / unmasked of the sums.
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def median(v):
    return sorted(v)[len(v) // 2]


def timed(fn, steps, warmup):
    times = []
    for i in range(warmup + steps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        if i >= warmup:
            times.append(e0.elapsed_time(e1))
    return dict(ms=median(times), min_ms=min(times), max_ms=max(times))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=16)
    ap.add_argument("--Lk", type=int, default=255)
    ap.add_argument("--fold", type=int, default=16)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "causal_attn_bench.py times kernels on a GPU"
    from item_alignment_amd import _lib
    lib = _lib.load()
    st = _lib.stream_ptr()
    B, Lk, fold, nh, H = a.B, a.Lk, a.fold, 1, 64
    Lq, scale = fold * Lk, 0.125
    bf, dev = torch.bfloat16, "cuda"
    g = torch.Generator(device="cpu").manual_seed(0)
    q = torch.randn(B * Lq, H, generator=g).to(bf).to(dev)
    kv = torch.randn(B * Lk, 2 * H, generator=g).to(bf).to(dev)
    dout = torch.randn(B * Lq, H, generator=g).to(bf).to(dev)
    out, dq, dkv = torch.empty_like(q), torch.empty_like(q), torch.empty_like(kv)
    lse = torch.empty(B * nh * Lq, dtype=torch.float32, device=dev)
    delta = torch.empty_like(lse)
    k_p, v_p, dk_p, dv_p = kv.data_ptr(), kv.data_ptr() + 2 * H, dkv.data_ptr(), dkv.data_ptr() + 2 * H

    def ok(rc, what):
        _lib.check(rc, what)

    def causal_fwd():
        ok(lib.ia_attn_fwd_causal_x(q.data_ptr(), H, k_p, v_p, 2 * H, out.data_ptr(), H, lse.data_ptr(), B, nh, Lk, fold, scale, st), "fwd causal")

    def causal_bwd():
        ok(lib.ia_attn_bwd_causal_x(q.data_ptr(), H, k_p, v_p, 2 * H, out.data_ptr(), dout.data_ptr(), H, lse.data_ptr(), delta.data_ptr(),
                                    dq.data_ptr(), H, dk_p, dv_p, 2 * H, B, nh, Lk, fold, scale, st), "bwd causal")

    def plain_fwd():
        ok(lib.ia_attn_fwd_x(q.data_ptr(), H, k_p, v_p, 2 * H, None, out.data_ptr(), H, lse.data_ptr(), B, nh, Lq, Lk, scale, 0.0, 0, st), "fwd x")

    def plain_bwd():
        ok(lib.ia_attn_bwd_x(q.data_ptr(), H, k_p, v_p, 2 * H, None, out.data_ptr(), dout.data_ptr(), H, lse.data_ptr(), delta.data_ptr(),
                             dq.data_ptr(), H, dk_p, dv_p, 2 * H, B, nh, Lq, Lk, scale, 0.0, 0, st), "bwd x")

    res = dict(B=B, Lk=Lk, fold=fold, nh=nh, Lq=Lq, steps=a.steps, warmup=a.warmup, gpu=torch.cuda.get_device_name(0))
    # each backward runs on the out / lse2 its own forward left behind
    plain = dict(fwd=timed(plain_fwd, a.steps, a.warmup), bwd=timed(plain_bwd, a.steps, a.warmup))
    causal = dict(fwd=timed(causal_fwd, a.steps, a.warmup), bwd=timed(causal_bwd, a.steps, a.warmup))
    for r in (plain, causal):
        r["fwd_bwd_ms"] = r["fwd"]["ms"] + r["bwd"]["ms"]
    res.update(unmasked_x=plain, causal_x=causal, causal_over_unmasked=causal["fwd_bwd_ms"] / plain["fwd_bwd_ms"])
    print(f"unmasked x form: fwd {plain['fwd']['ms']:.3f} ms + bwd {plain['bwd']['ms']:.3f} ms = {plain['fwd_bwd_ms']:.3f} ms; "
          f"causal: fwd {causal['fwd']['ms']:.3f} ms + bwd {causal['bwd']['ms']:.3f} ms = {causal['fwd_bwd_ms']:.3f} ms; "
          f"causal / unmasked = {res['causal_over_unmasked']:.2f}", flush=True)
    print(json.dumps(res))
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
