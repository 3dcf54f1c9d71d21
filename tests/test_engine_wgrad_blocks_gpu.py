"""ia_layer_bwd2 of a post-LN layer with the weight gradients on the 32-row block mask (ia_kblock_mask): the "wide" configuration of
tests/test_engine_wgrad_rows_gpu.py (H 1024, I 4096, B 32, L 255: all four weight gradients take the 256-wide kernel), three ways --
(a) masked_rows_dead = 0, (b) masked with the mask the call builds itself, (c) masked with a caller's ia_kblock_mask_host mask in
ia_layer_cfg::key_rows.kblocks -- and every gradient and dx equal bit for bit across the three.  (d) The same walk through the entry
that takes the rows' live bytes, at the same width: ia_gemm_wgrad_rows over the key mask on the operands of (a)'s QKV weight gradient (its
dy as the backward left it in the scratch, and x) gives (a)'s gradient bit for bit.

In (b) and (c) the scratch is filled with 0xFF bytes (bf16 NaN everywhere) before the call: nothing the backward reads there may be left
over from before the call.  The layer input x -- read by the QKV weight gradient
only -- is also overwritten with infinities in the rows of dead 32-row blocks, the dead halves of partly live k-tiles included: only a
walk over 32-row blocks returns the clean result.  One more case runs a layer with out_row_live and a caller's out_rows.kblocks."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

BLK = 32
NH, L = 16, 255
H, I = NH * 64, NH * 256
LENGTHS = [255, 64, 27, 130, 200, 9, 255, 101]


def host_mask(live, M):
    """ia_kblock_mask_host words of a uint8 row mask on the GPU, as a GPU tensor"""
    from item_alignment_amd import _lib
    lib = _lib.load()
    live_np = np.ascontiguousarray(live.view(-1).cpu().numpy())
    kb = np.zeros(lib.ia_kblock_mask_bytes(M) // 4, np.int32)
    assert lib.ia_kblock_mask_host(live_np.ctypes.data, M, kb.ctypes.data) == 0
    return torch.from_numpy(kb).to(live.device)


def setup(gpu, B):
    from item_alignment_amd import _lib
    from item_alignment_amd._lib import LayerWeights
    from test_engine_gpu import make_layer
    lib = _lib.load()
    M = B * L
    assert [lib.ia_gemm_wgrad_rows_filters(no, ni, M) for no, ni in ((H, I), (I, H), (H, H), (3 * H, H))] == [1, 1, 1, 1]
    P32 = make_layer(H, I, gpu, 3)
    mats = ("w_qkv", "w_o", "w_fc1", "w_fc2")
    Pb = {k: v.to(torch.bfloat16) for k, v in P32.items() if k in mats}
    w = LayerWeights()
    for k in P32:
        setattr(w, k, (Pb[k] if k in mats else P32[k]).data_ptr())
    x = torch.randn(B, L, H, generator=torch.Generator().manual_seed(5)).to(gpu).to(torch.bfloat16).view(M, H)
    lens = torch.tensor([LENGTHS[i % len(LENGTHS)] for i in range(B)])
    mask = (torch.arange(L)[None] < lens[:, None]).to(torch.uint8).to(gpu).contiguous()
    return lib, P32, (Pb, w), x, mask


def run_bwd(lib, P32, w, cfg, x_in, mask, y, stash, dy, poison):
    from item_alignment_amd import _lib
    from item_alignment_amd._lib import LayerGrads
    gpu = dy.device
    scratch = torch.full((lib.ia_layer_bwd_scratch_bytes(C.byref(cfg)),), 0xFF if poison else 0, device=gpu, dtype=torch.uint8)
    G = {k: torch.zeros_like(v) for k, v in P32.items()}
    g = LayerGrads()
    for k in P32:
        setattr(g, k, G[k].data_ptr())
    dx = torch.full_like(dy, float("nan"))
    _lib.check(lib.ia_layer_bwd2(C.byref(cfg), C.byref(w), C.byref(g), x_in.data_ptr(), mask.data_ptr(), y.data_ptr(), stash.data_ptr(),
                                 dy.data_ptr(), None, dx.data_ptr(), None, scratch.data_ptr(), scratch.numel(), torch.cuda.current_stream().cuda_stream),
               f"bwd2 (masked_rows_dead={cfg.masked_rows_dead})")
    torch.cuda.synchronize()
    return dx, G, scratch


def al(b):
    return (b + 255) // 256 * 256


def assert_same(ref, got, P32, what):
    assert torch.isfinite(got[0].float()).all(), what
    assert torch.equal(ref[0], got[0]), what
    for k in P32:
        assert torch.isfinite(got[1][k]).all(), (what, k)
        assert torch.equal(ref[1][k], got[1][k]), (what, k)


@pytest.mark.parametrize("drop", [0.0, 0.1])
def test_layer_bwd2_block_mask_equals_dense(gpu, drop):
    from item_alignment_amd import _lib
    from item_alignment_amd._lib import LayerCfg
    B = 32
    M = B * L
    lib, P32, (Pb, w), x, mask = setup(gpu, B)
    valid = mask.bool().view(-1)
    dy = torch.randn(M, H, generator=torch.Generator().manual_seed(6)).to(gpu).to(torch.bfloat16)
    dy = (dy * valid[:, None].to(dy.dtype)).contiguous()          # zero at masked positions: what masked_rows_dead promises
    cfg = lambda flag: LayerCfg(B=B, L=L, H=H, I=I, nh=NH, pre_ln=0, eps=1e-12, hidden_drop=drop, attn_drop=drop, seed=11, layer_id=2,
                                masked_rows_dead=flag)
    c0 = cfg(0)
    stash = torch.empty(lib.ia_layer_stash_bytes(C.byref(c0)), device=gpu, dtype=torch.uint8)
    y = torch.empty(M, H, device=gpu, dtype=torch.bfloat16)
    _lib.check(lib.ia_layer_fwd(C.byref(c0), C.byref(w), x.data_ptr(), mask.data_ptr(), y.data_ptr(), stash.data_ptr(),
                                torch.cuda.current_stream().cuda_stream), "fwd")
    kb = host_mask(mask, M)

    def variant(which, x_in):
        c = cfg(0 if which == "a" else 1)
        if which == "c":
            c.key_rows.kblocks = kb.data_ptr()
        return run_bwd(lib, P32, w, c, x_in, mask, y, stash, dy, poison=which in "bc")

    a = variant("a", x)
    for k in P32:
        assert a[1][k].abs().max().item() > 0.0, k
    for which in "bc":
        assert_same(a, variant(which, x), P32, which)
    # (d) the QKV weight gradient's dy: the fifth buffer of carve_scratch (engine.hip), behind three [M, H] and one [M, I]
    off = 3 * al(M * H * 2) + al(M * I * 2)
    gqkv = a[2][off: off + M * 3 * H * 2].view(torch.bfloat16).view(M, 3 * H)
    assert gqkv[valid].float().abs().max().item() > 0.0 and gqkv[~valid].float().abs().max().item() == 0.0
    assert lib.ia_gemm_wgrad_rows_filters(3 * H, H, M) == 1
    ws = torch.full((lib.ia_gemm_wgrad_rows_workspace_bytes(3 * H, H, M),), 0xFF, device=gpu, dtype=torch.uint8)
    dw = torch.zeros_like(a[1]["w_qkv"])
    _lib.check(lib.ia_gemm_wgrad_rows(gqkv.data_ptr(), 3 * H, x.data_ptr(), H, dw.data_ptr(), H, 3 * H, H, M, mask.data_ptr(), 1, ws.data_ptr(),
                                      ws.numel(), torch.cuda.current_stream().cuda_stream), "ia_gemm_wgrad_rows")
    torch.cuda.synchronize()
    assert torch.isfinite(dw).all() and torch.equal(dw, a[1]["w_qkv"]), "d"
    # infinities in x in the rows of every dead 32-row block
    nb = (M + BLK - 1) // BLK
    pad = torch.zeros(nb * BLK, dtype=torch.bool, device=gpu)
    pad[:M] = valid
    blk_dead = ~pad.view(nb, BLK).any(1)
    dead_rows = blk_dead.repeat_interleave(BLK)[:M]
    halves = torch.cat([blk_dead, blk_dead.new_ones(nb % 2)]).view(-1, 2)
    half_dead = (halves.sum(1) == 1).sum().item()      # k-tiles with exactly one dead half: what a walk over whole k-tiles would read
    assert dead_rows.sum().item() >= 40 * BLK and half_dead >= 8
    xp = x.clone()
    xp[dead_rows] = float("inf")
    for which in "bc":
        assert_same(a, variant(which, xp), P32, which + " with infinities in x")


def test_layer_bwd2_out_row_live_block_mask(gpu):
    """out_row_live (row 0 of each sequence) on a post-LN layer: a caller's block mask (out_rows.kblocks) against the same call building
    its own mask"""
    from item_alignment_amd import _lib
    from item_alignment_amd._lib import LayerCfg
    B = 32
    M = B * L
    lib, P32, (Pb, w), x, mask = setup(gpu, B)
    live = torch.zeros(B, L, dtype=torch.uint8, device=gpu)
    live[:, 0] = mask[:, 0]
    live = live.view(-1).contiguous()
    assert live.sum().item() == B
    dy = torch.randn(M, H, generator=torch.Generator().manual_seed(6)).to(gpu).to(torch.bfloat16)
    dy = (dy * live[:, None].to(dy.dtype)).contiguous()           # zero outside out_row_live: the contract
    kb = host_mask(live, M)

    def cfg(flag, okb):
        c = LayerCfg(B=B, L=L, H=H, I=I, nh=NH, pre_ln=0, eps=1e-12, hidden_drop=0.1, attn_drop=0.1, seed=11, layer_id=2, masked_rows_dead=flag)
        c.out_row_live = live.data_ptr()
        c.out_rows.kblocks = None if okb is None else okb.data_ptr()
        return c
    cf = cfg(3, None)
    stash = torch.empty(lib.ia_layer_stash_bytes(C.byref(cf)), device=gpu, dtype=torch.uint8)
    y = torch.empty(M, H, device=gpu, dtype=torch.bfloat16)
    _lib.check(lib.ia_layer_fwd(C.byref(cf), C.byref(w), x.data_ptr(), mask.data_ptr(), y.data_ptr(), stash.data_ptr(),
                                torch.cuda.current_stream().cuda_stream), "fwd")
    ref = run_bwd(lib, P32, w, cf, x, mask, y, stash, dy, poison=False)
    for k in P32:
        assert ref[1][k].abs().max().item() > 0.0, k
    assert_same(ref, run_bwd(lib, P32, w, cfg(3, kb), x, mask, y, stash, dy, poison=True), P32, "caller's kblocks")
    assert_same(ref, run_bwd(lib, P32, w, cfg(3, None), x, mask, y, stash, dy, poison=True), P32, "own mask, scratch poisoned")
