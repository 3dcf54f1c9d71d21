"""ia_layer_bwd2 of a post-LN layer with ia_layer_cfg::masked_rows_dead: the three plain data gradients (fc1, out-projection, QKV) run over
the live 32-row blocks only (one block list per call, built into the scratch) and every gradient stays what the same backward returns
with the list withheld (ia_debug_dgrad_rows(0): the unfiltered data-gradient calls, every other row filter in place).  The x gelu' +
column sums gradient (fc2) runs every row in the engine, so the fc1 bias gradient is bit-identical too.

B = 40, H = 1024, nh = 16, I = 1024: the smallest layer whose four data gradients all reach the 256-wide kernel (160 tiles of 256 x 256
at L = 255; asserted through ia_gemm_dgrad_rows_filters), dropout on, ragged right-padded masks, the backward scratch filled with NaN
bit patterns before each call.  L = 255 runs the one-pass attention backward (which skips dead 32-query blocks but reads the padded
rows of partly live ones); L = 300 puts the pair kernels, which read every row of d_o, behind the filtered out-projection gradient.
"split" hands dx2 to the call (the last data gradient has the plain epilogue), "fused" does not (it adds dz1: IA_EPI_ADD).  Weights are
read k-strided or through their transposed copies (ia_layer_weights::wt_*), the form the towers use.

Everything must compare equal, the fc1 bias gradient included; it is also held to the bound of tests/test_gemm_dgrad_rows_gpu.py:
against the fp64 column sum of the bf16 gradient it sums (gI, read back from the scratch) the filtered error may be at most twice the
unfiltered one."""
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu

B, NH, H, I = 40, 16, 1024, 1024
LENGTHS = [255, 64, 27, 130, 200, 9, 255, 101, 33, 180]


@pytest.mark.parametrize("L,form,shadows", [(255, "split", True), (255, "fused", False), (300, "split", True)])
def test_layer_bwd2_filtered_dgrad_equals_unfiltered(gpu, L, form, shadows):
    from item_alignment_amd import _lib
    from item_alignment_amd._lib import LayerCfg, LayerGrads, LayerWeights
    from test_engine_gpu import make_layer
    lib = _lib.load()
    M = B * L
    assert [lib.ia_gemm_dgrad_rows_filters(M, n, k) for n, k in ((I, H), (H, I), (H, H), (H, 3 * H))] == [1, 1, 1, 1]
    P32 = make_layer(H, I, gpu, 3)
    mats = ("w_qkv", "w_o", "w_fc1", "w_fc2")
    Pb = {k: v.to(torch.bfloat16) for k, v in P32.items() if k in mats}
    Pt = {k: v.t().contiguous() for k, v in Pb.items()}
    x = torch.randn(B, L, H, generator=torch.Generator().manual_seed(5)).to(gpu).to(torch.bfloat16)
    lens = torch.tensor([min(L, LENGTHS[i % len(LENGTHS)] + (L - 255 if i % 3 == 0 else 0)) for i in range(B)])
    mask = (torch.arange(L)[None] < lens[:, None]).to(torch.uint8).to(gpu)
    valid = mask.bool().view(-1)
    dy = torch.randn(M, H, generator=torch.Generator().manual_seed(6)).to(gpu).to(torch.bfloat16)
    dy = (dy * valid[:, None].to(dy.dtype)).contiguous()          # zero at masked positions: what masked_rows_dead promises
    w = LayerWeights()
    for k in P32:
        setattr(w, k, (Pb[k] if k in mats else P32[k]).data_ptr())
    if shadows:
        for k in mats:
            setattr(w, "wt_" + k[2:], Pt[k].data_ptr())
    st = torch.cuda.current_stream().cuda_stream
    cfg = LayerCfg(B=B, L=L, H=H, I=I, nh=NH, pre_ln=0, eps=1e-12, hidden_drop=0.1, attn_drop=0.1, seed=11, layer_id=2, masked_rows_dead=1)
    stash = torch.empty(lib.ia_layer_stash_bytes(C.byref(cfg)), device=gpu, dtype=torch.uint8)
    y = torch.empty(M, H, device=gpu, dtype=torch.bfloat16)
    _lib.check(lib.ia_layer_fwd(C.byref(cfg), C.byref(w), x.data_ptr(), mask.data_ptr(), y.data_ptr(), stash.data_ptr(), st), "fwd")

    def backward(filtered):
        scratch = torch.full((lib.ia_layer_bwd_scratch_bytes(C.byref(cfg)),), 0xFF, device=gpu, dtype=torch.uint8)      # NaN as bf16 and as fp32
        G = {k: torch.zeros_like(v) for k, v in P32.items()}
        g = LayerGrads()
        for k in P32:
            setattr(g, k, G[k].data_ptr())
        dx = torch.full_like(dy, float("nan"))
        dx2 = torch.full_like(dy, float("nan")) if form == "split" else None
        was = lib.ia_debug_dgrad_rows(1 if filtered else 0)
        try:
            _lib.check(lib.ia_layer_bwd2(C.byref(cfg), C.byref(w), C.byref(g), x.data_ptr(), mask.data_ptr(), y.data_ptr(), stash.data_ptr(),
                                         dy.data_ptr(), None, dx.data_ptr(), dx2.data_ptr() if dx2 is not None else None,
                                         scratch.data_ptr(), scratch.numel(), st), f"bwd2 (filtered={filtered})")
            torch.cuda.synchronize()
        finally:
            lib.ia_debug_dgrad_rows(was)
        al = lambda b: (b + 255) // 256 * 256
        gI = scratch[3 * al(M * H * 2): 3 * al(M * H * 2) + M * I * 2].view(torch.bfloat16).view(M, I)      # carve order: g0, g1, g2, gI
        return dx, dx2, G, gI.clone()

    plain, filt = backward(False), backward(True)
    for name, a, b in (("dx", plain[0], filt[0]), ("dx2", plain[1], filt[1])):
        if a is None:
            continue
        assert torch.isfinite(b.float()).all(), name
        assert torch.equal(a, b), name
    assert filt[0][~valid].abs().max().item() == 0.0               # dead rows leave as zeros
    assert torch.isfinite(filt[3].float()).all() and torch.equal(plain[3], filt[3])
    for k in P32:
        assert plain[2][k].abs().max().item() > 0.0, k
        assert torch.equal(plain[2][k], filt[2][k]), k
    ref = filt[3].cpu().double().sum(0)
    e_f = (filt[2]["b_fc1"].cpu().double() - ref).abs().max().item()
    e_d = (plain[2]["b_fc1"].cpu().double() - ref).abs().max().item()
    print(f"L {L} {form}: fc1 bias gradient vs fp64: filtered {e_f:.3e}, unfiltered {e_d:.3e}")
    assert e_f <= 2.0 * e_d, (e_f, e_d)
