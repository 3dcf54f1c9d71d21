"""ia_layer_bwd2 of a post-LN layer with ia_layer_cfg::masked_rows_dead: the four weight gradients go through the row-filtered GEMM
(one bitmask of the live 32-row blocks per call, built into the scratch) and every gradient stays what the dense backward (masked_rows_dead = 0)
returns, bit for bit, with dropout on and off.

Two configurations.  "small": B = 3 sequences of L = 255 with lengths 255, 64 and 27 (a full row, a padding that starts on a 64-row tile
boundary, a nearly empty row) at nh = 2, the smallest post-LN layer of tests/test_engine_gpu.py -- its weight gradients are 128 wide, take
the 128-wide kernel and read every row, so it checks the plumbing only.  "wide": H = 1024, I = 4096, B = 32 (the same three lengths among
them): all four weight gradients take the 256-wide kernel and honour the bitmask (asserted through ia_gemm_wgrad_rows_filters), so the
scratch carve of the mask, the helper's shapes and the one-mask-for-four-GEMMs reuse are what the equality checks.  There the layer input x
-- which the backward reads in the QKV weight gradient only -- is also overwritten with infinities in the rows of k-tiles that are dead as a
whole (tests/test_engine_wgrad_blocks_gpu.py does the same for every dead 32-row block): a GEMM that read them would turn 0 x inf into NaN."""
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu

BK = 64
CONFIGS = {"small": (3, 2, [255, 64, 27]), "wide": (32, 16, [255, 64, 27, 130, 200, 9, 255, 101])}


@pytest.mark.parametrize("drop", [0.0, 0.1])
@pytest.mark.parametrize("config", ["small", "wide"])
def test_layer_bwd2_masked_rows_dead_equals_dense(gpu, config, drop):
    from item_alignment_amd import _lib
    from item_alignment_amd._lib import LayerCfg, LayerGrads, LayerWeights
    from test_engine_gpu import make_layer
    lib = _lib.load()
    B, nh, some = CONFIGS[config]
    L = 255
    H, I, M = nh * 64, nh * 256, B * L
    filters = [lib.ia_gemm_wgrad_rows_filters(n_out, n_in, M) for n_out, n_in in ((H, I), (I, H), (H, H), (3 * H, H))]
    assert filters == ([1, 1, 1, 1] if config == "wide" else [0, 0, 0, 0])      # "wide" must reach the filtering kernel in all four
    P32 = make_layer(H, I, gpu, 3)
    mats = ("w_qkv", "w_o", "w_fc1", "w_fc2")
    Pb = {k: v.to(torch.bfloat16) for k, v in P32.items() if k in mats}
    x = torch.randn(B, L, H, generator=torch.Generator().manual_seed(5)).to(gpu).to(torch.bfloat16)
    lens = torch.tensor([some[i % len(some)] for i in range(B)])
    mask = (torch.arange(L)[None] < lens[:, None]).to(torch.uint8).to(gpu)
    valid = mask.bool().view(-1)
    dy = torch.randn(M, H, generator=torch.Generator().manual_seed(6)).to(gpu).to(torch.bfloat16)
    dy = (dy * valid[:, None].to(dy.dtype)).contiguous()          # zero at masked positions: what masked_rows_dead promises
    w = LayerWeights()
    for k in P32:
        setattr(w, k, (Pb[k] if k in mats else P32[k]).data_ptr())
    st = torch.cuda.current_stream().cuda_stream
    cfg = lambda flag: LayerCfg(B=B, L=L, H=H, I=I, nh=nh, pre_ln=0, eps=1e-12, hidden_drop=drop, attn_drop=drop, seed=11, layer_id=2,
                                masked_rows_dead=flag)
    c0 = cfg(0)
    stash = torch.empty(lib.ia_layer_stash_bytes(C.byref(c0)), device=gpu, dtype=torch.uint8)
    y = torch.empty(M, H, device=gpu, dtype=torch.bfloat16)
    _lib.check(lib.ia_layer_fwd(C.byref(c0), C.byref(w), x.data_ptr(), mask.data_ptr(), y.data_ptr(), stash.data_ptr(), st), "fwd")

    def backward(flag, x_in):
        cf = cfg(flag)
        scratch = torch.empty(lib.ia_layer_bwd_scratch_bytes(C.byref(cf)), device=gpu, dtype=torch.uint8)
        G = {k: torch.zeros_like(v) for k, v in P32.items()}
        g = LayerGrads()
        for k in P32:
            setattr(g, k, G[k].data_ptr())
        dx = torch.empty_like(dy)
        _lib.check(lib.ia_layer_bwd2(C.byref(cf), C.byref(w), C.byref(g), x_in.data_ptr(), mask.data_ptr(), y.data_ptr(), stash.data_ptr(),
                                     dy.data_ptr(), None, dx.data_ptr(), None, scratch.data_ptr(), scratch.numel(), st),
                   f"bwd2 (masked_rows_dead={flag})")
        torch.cuda.synchronize()
        return dx, G

    dense, filt = backward(0, x), backward(1, x)
    assert torch.isfinite(filt[0].float()).all()
    assert torch.equal(dense[0], filt[0])
    for k in P32:
        assert dense[1][k].abs().max().item() > 0.0, k
        assert torch.equal(dense[1][k], filt[1][k]), k
    if config == "wide":
        nk = (M + BK - 1) // BK
        pad = torch.zeros(nk * BK, dtype=torch.bool, device=gpu)
        pad[:M] = valid
        dead_rows = (~pad.view(nk, BK).any(1)).repeat_interleave(BK)[:M]
        assert dead_rows.view(-1).sum().item() >= 20 * BK              # the short sequences leave whole k-tiles of padding
        xp = x.view(M, H).clone()
        xp[dead_rows] = float("inf")
        dxp, Gp = backward(1, xp)
        assert torch.equal(Gp["w_qkv"], filt[1]["w_qkv"])
        assert torch.equal(dxp, filt[0])
