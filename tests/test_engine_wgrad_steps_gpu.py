"""ia_layer_bwd2 with the weight gradients on the walk over live 16-row steps (ia_kstep_mask, built by the call in the last slots of its
scratch): one post-LN layer under masked_rows_dead with a ragged key mask, and one pre-LN layer with out_row_live, each against the same
layer with every row computed -- dx, dx2 and every parameter gradient bit for bit, everything finite.  The filtered calls start from a
stash, a scratch and outputs filled with 0xFF bytes (NaN as bf16 and as fp32).

The shapes are the narrowest of the engine tests at which all the filtered weight gradients of the layer take the step walk
(ia_gemm_wgrad_walk == 2): H 1024, I 4096, 32 x 255 rows, and the ViT block's H 768, I 3072, 24 x 577 rows."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

STEP = 16
BF = torch.bfloat16
TXT = dict(B=32, L=255, H=1024, NH=16, I=4096, pre_ln=0)
VIT = dict(B=24, L=577, H=768, NH=12, I=3072, pre_ln=1)
LENGTHS = [255, 1, 64, 27, 130, 200, 9, 101, 33, 180]


def al(b):
    return (b + 255) // 256 * 256


def numpy_steps(live_np):
    n = (len(live_np) + STEP - 1) // STEP
    bits = np.array([live_np[t * STEP: (t + 1) * STEP].any() for t in range(n)] + [False] * (-n % 32))
    return (bits.reshape(-1, 32) * (1 << np.arange(32, dtype=np.uint64))).sum(1).astype(np.uint32)


@pytest.mark.parametrize("shape", ["txt", "vit"])
def test_layer_bwd2_step_walk_equals_every_row_call(gpu, shape):
    from item_alignment_amd import _lib
    from item_alignment_amd._lib import LayerCfg, LayerGrads, LayerWeights
    from test_engine_gpu import make_layer
    lib = _lib.load()
    s = VIT if shape == "vit" else TXT
    B, L, H, I, NH, pre_ln = s["B"], s["L"], s["H"], s["I"], s["NH"], s["pre_ln"]
    M = B * L
    filtered = ((H, I), (I, H), (H, H)) + (() if pre_ln else ((3 * H, H),))      # (a pre-LN layer's QKV weight gradient sees every row)
    assert [lib.ia_gemm_wgrad_walk(no, ni, M) for no, ni in filtered] == [2] * len(filtered)
    P32 = make_layer(H, I, gpu, 3)
    mats = ("w_qkv", "w_o", "w_fc1", "w_fc2")
    Pb = {k: v.to(BF) for k, v in P32.items() if k in mats}
    w = LayerWeights()
    for k in P32:
        setattr(w, k, (Pb[k] if k in mats else P32[k]).data_ptr())
    x = torch.randn(M, H, generator=torch.Generator().manual_seed(5)).to(gpu).to(BF)
    if pre_ln:      # no key mask; the head reads row 0 of each sequence
        mask, live = None, torch.zeros(M, dtype=torch.uint8)
        live[::L] = 1
        live = live.to(gpu)
    else:           # right-padded sequences: the rows behind a sequence's length are dead
        lens = torch.tensor([LENGTHS[i % len(LENGTHS)] for i in range(B)])
        mask = (torch.arange(L)[None] < lens[:, None]).to(torch.uint8).to(gpu).contiguous()
        live = mask.view(-1)
    lv = live.bool()
    n_steps = (M + STEP - 1) // STEP
    live_np = np.ascontiguousarray(live.cpu().numpy())
    partly = sum(0 < live_np[t * STEP: (t + 1) * STEP].sum() < min(STEP, M - t * STEP) for t in range(n_steps))
    dead = sum(not live_np[t * STEP: (t + 1) * STEP].any() for t in range(n_steps))
    assert partly >= B // 2 and dead >= n_steps // 4               # both kinds of step: partly live ones and whole dead ones
    dy = torch.randn(M, H, generator=torch.Generator().manual_seed(6)).to(gpu).to(BF)
    dy = (dy * live[:, None].to(BF)).contiguous()                    # zero in the dead rows: the contract
    drop = 0.0 if pre_ln else 0.1
    base = dict(B=B, L=L, H=H, I=I, nh=NH, pre_ln=pre_ln, eps=1e-6 if pre_ln else 1e-12, hidden_drop=drop, attn_drop=drop, seed=11, layer_id=2)
    cfg_d, cfg_f = LayerCfg(masked_rows_dead=0, **base), LayerCfg(masked_rows_dead=0 if pre_ln else 3, **base)
    if pre_ln:
        cfg_f.out_row_live = live.data_ptr()
    mp = None if mask is None else mask.data_ptr()
    st = torch.cuda.current_stream().cuda_stream

    def step(cfg, poison):
        fillv = 0xFF if poison else 0
        stash = torch.full((lib.ia_layer_stash_bytes(C.byref(cfg)),), fillv, device=gpu, dtype=torch.uint8)
        y = torch.full((M, H), -1 if poison else 0, device=gpu, dtype=torch.int16).view(BF)
        _lib.check(lib.ia_layer_fwd(C.byref(cfg), C.byref(w), x.data_ptr(), mp, y.data_ptr(), stash.data_ptr(), st), "fwd")
        scratch = torch.full((lib.ia_layer_bwd_scratch_bytes(C.byref(cfg)),), fillv, device=gpu, dtype=torch.uint8)
        G = {k: torch.zeros_like(v) for k, v in P32.items()}
        g = LayerGrads()
        for k in P32:
            setattr(g, k, G[k].data_ptr())
        dx = torch.full((M, H), -1 if poison else 0, device=gpu, dtype=torch.int16).view(BF)
        dx2 = None if pre_ln else torch.full((M, H), -1 if poison else 0, device=gpu, dtype=torch.int16).view(BF)
        _lib.check(lib.ia_layer_bwd2(C.byref(cfg), C.byref(w), C.byref(g), x.data_ptr(), mp, y.data_ptr(), stash.data_ptr(), dy.data_ptr(), None,
                                     dx.data_ptr(), None if dx2 is None else dx2.data_ptr(), scratch.data_ptr(), scratch.numel(), st), "bwd2")
        torch.cuda.synchronize()
        return dict(dx=dx, dx2=dx2, G=G, scratch=scratch)

    d, f = step(cfg_d, False), step(cfg_f, True)
    for name in ("dx", "dx2"):
        if d[name] is None:
            continue
        assert torch.isfinite(f[name].float()).all(), name
        assert d[name].float().abs().max().item() > 0, name
        assert torch.equal(f[name], d[name]), name
    for k in P32:
        assert torch.isfinite(f["G"][k]).all(), k
        assert d["G"][k].abs().max().item() > 0.0, k
        assert torch.equal(f["G"][k], d["G"][k]), k
    # the step mask the call built: the last two slots of the scratch are the key mask's and out_row_live's
    slot = al(lib.ia_kstep_mask_bytes(M))
    words = lib.ia_kstep_mask_bytes(M) // 4
    tail = f["scratch"][-2 * slot:].cpu().numpy()
    built = tail[slot: slot + 4 * words] if pre_ln else tail[: 4 * words]
    assert np.array_equal(built.view(np.uint32), numpy_steps(live_np))
