"""ia_layer_fwd / ia_layer_fwd_infer of a post-LN layer with ia_layer_cfg::masked_rows_dead = 3: the four GEMMs of the forward run over
the live 32-row blocks only and the two LayerNorms over the live rows only, and everything a caller can observe at an unmasked position
stays what the dense forward (ia_debug_fwd_rows(0), same flag) gives -- bit for bit.

The layer of tests/test_engine_dgrad_rows_gpu.py: B = 40, H = 1024, nh = 16, I = 1024 (the smallest layer whose GEMMs all reach the
256-wide kernel, asserted through ia_gemm_fwd_rows_filters), its LENGTHS, L = 255 and 300 (M = 10200 and 12000: neither a multiple of
128, so the QKV projection's scaled columns meet the guarded epilogue on their last rows), dropout 0.1.  Stash and y are filled with
0xFF (NaN as bf16 and as fp32) before each forward.

Checks: y and every stash buffer are equal at the live rows and finite everywhere; ia_layer_bwd2 from each of the two stashes, with dy
zero at the masked positions, returns torch.equal dx, dx2 and parameter gradients; ia_layer_fwd_infer agrees on y in the same way.  One
case hands the calls the block list and the block mask from the host builders (ia_layer_cfg::key_rows.blocks / .kblocks), the others
leave them NULL (the engine builds its own): same results."""
import ctypes as C

import numpy as np
import pytest
import torch

from test_engine_dgrad_rows_gpu import B, H, I, LENGTHS, NH

pytestmark = pytest.mark.gpu


def al(b):
    return (b + 255) // 256 * 256


def stash_views(stash, M, L):
    """the buffers of carve_stash (engine.hip) by name, in carve order"""
    sizes = [("qkv", M * 3 * H * 2, torch.bfloat16, (M, 3 * H)), ("ctx", M * H * 2, torch.bfloat16, (M, H)), ("z1", M * H * 2, torch.bfloat16, (M, H)),
             ("y1", M * H * 2, torch.bfloat16, (M, H)), ("z2", M * H * 2, torch.bfloat16, (M, H)), ("hpre", M * I * 2, torch.bfloat16, (M, I)),
             ("hact", M * I * 2, torch.bfloat16, (M, I)), ("lse", B * NH * L * 4, torch.float32, (B, NH, L)), ("mean1", M * 4, torch.float32, (M,)),
             ("rstd1", M * 4, torch.float32, (M,)), ("mean2", M * 4, torch.float32, (M,)), ("rstd2", M * 4, torch.float32, (M,))]
    out, off = {}, 0
    for name, nbytes, dt, shape in sizes:
        out[name] = stash[off: off + nbytes].view(dt).view(shape)
        off += al(nbytes)
    return out


@pytest.mark.parametrize("L,host_lists", [(255, False), (255, True), (300, False)])
def test_layer_forward_row_skip_equals_dense(gpu, L, host_lists):
    from item_alignment_amd import _lib
    from item_alignment_amd._lib import LayerCfg, LayerGrads, LayerWeights
    from test_engine_gpu import make_layer
    lib = _lib.load()
    M = B * L
    assert [lib.ia_gemm_fwd_rows_filters(M, n, k) for n, k in ((3 * H, H), (H, H), (I, H), (H, I))] == [1, 1, 1, 1]
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
    for k in mats:
        setattr(w, "wt_" + k[2:], Pt[k].data_ptr())
    st = torch.cuda.current_stream().cuda_stream
    cfg = LayerCfg(B=B, L=L, H=H, I=I, nh=NH, pre_ln=0, eps=1e-12, hidden_drop=0.1, attn_drop=0.1, seed=11, layer_id=2, masked_rows_dead=3)
    lists = None
    if host_lists:
        live_np = np.ascontiguousarray(mask.view(-1).cpu().numpy())
        rb = np.zeros(lib.ia_row_blocks_bytes(M) // 4, np.int32)
        kb = np.zeros(lib.ia_kblock_mask_bytes(M) // 4, np.int32)
        assert lib.ia_row_blocks_host(live_np.ctypes.data, M, rb.ctypes.data) == 0
        assert lib.ia_kblock_mask_host(live_np.ctypes.data, M, kb.ctypes.data) == 0
        lists = (torch.from_numpy(rb).to(gpu), torch.from_numpy(kb).to(gpu))
        cfg.key_rows.blocks, cfg.key_rows.kblocks = lists[0].data_ptr(), lists[1].data_ptr()

    def forward(skip):
        stash = torch.full((lib.ia_layer_stash_bytes(C.byref(cfg)),), 0xFF, device=gpu, dtype=torch.uint8)
        y = torch.full((M, H), -1, device=gpu, dtype=torch.int16).view(torch.bfloat16)
        yi = torch.full((M, H), -1, device=gpu, dtype=torch.int16).view(torch.bfloat16)
        scratch = torch.full((lib.ia_layer_infer_scratch_bytes(C.byref(cfg)),), 0xFF, device=gpu, dtype=torch.uint8)
        was = lib.ia_debug_fwd_rows(1 if skip else 0)
        try:
            _lib.check(lib.ia_layer_fwd(C.byref(cfg), C.byref(w), x.data_ptr(), mask.data_ptr(), y.data_ptr(), stash.data_ptr(), st), f"fwd (skip={skip})")
            _lib.check(lib.ia_layer_fwd_infer(C.byref(cfg), C.byref(w), x.data_ptr(), mask.data_ptr(), yi.data_ptr(), scratch.data_ptr(),
                                              scratch.numel(), st), f"fwd_infer (skip={skip})")
            torch.cuda.synchronize()
        finally:
            lib.ia_debug_fwd_rows(was)
        return y, yi, stash

    def backward(stash, y):
        scratch = torch.full((lib.ia_layer_bwd_scratch_bytes(C.byref(cfg)),), 0xFF, device=gpu, dtype=torch.uint8)
        G = {k: torch.zeros_like(v) for k, v in P32.items()}
        g = LayerGrads()
        for k in P32:
            setattr(g, k, G[k].data_ptr())
        dx = torch.full_like(dy, float("nan"))
        dx2 = torch.full_like(dy, float("nan"))
        _lib.check(lib.ia_layer_bwd2(C.byref(cfg), C.byref(w), C.byref(g), x.data_ptr(), mask.data_ptr(), y.data_ptr(), stash.data_ptr(),
                                     dy.data_ptr(), None, dx.data_ptr(), dx2.data_ptr(), scratch.data_ptr(), scratch.numel(), st), "bwd2")
        torch.cuda.synchronize()
        return dx, dx2, G

    y_d, yi_d, stash_d = forward(False)
    y_s, yi_s, stash_s = forward(True)
    for name, a, b in (("y", y_d, y_s), ("y infer", yi_d, yi_s)):
        assert torch.isfinite(b.float()).all(), name
        assert torch.equal(a[valid], b[valid]), name
        assert b[~valid].float().abs().max().item() == 0.0, name          # masked positions leave as zeros
    vd, vs = stash_views(stash_d, M, L), stash_views(stash_s, M, L)
    for name in vd:
        a, b = vd[name], vs[name]
        assert torch.isfinite(b.float()).all(), name                      # the backward reads every row of some of them
        if name == "lse":
            live = mask.bool()[:, None, :].expand(B, NH, L)
            assert torch.equal(a[live], b[live]), name
        else:
            assert torch.equal(a[valid], b[valid]), name
    dense, skip = backward(stash_d, y_d), backward(stash_s, y_s)
    for name, a, b in (("dx", dense[0], skip[0]), ("dx2", dense[1], skip[1])):
        assert torch.isfinite(b.float()).all(), name
        assert torch.equal(a, b), name
    for k in P32:
        assert dense[2][k].abs().max().item() > 0.0, k
        assert torch.equal(dense[2][k], skip[2][k]), k
    del lists
