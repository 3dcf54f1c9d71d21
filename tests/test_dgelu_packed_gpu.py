"""The x gelu' + column-sums data gradient over the block-packed list (ia_row_groups_packed, ia_gemm_dgrad_packed): the live 32-row blocks of
a ragged key mask packed by whole 128-row groups, and the fc1 bias gradient still BIT-IDENTICAL to the dense call's (torch.equal).

Shape: M = 10 x 255 = 2 550 rows (no multiple of 32), N_in = 4096, K_out = 128 -- 10 x 16 = 160 tiles, the smallest plan at which the dense
call takes the 256-wide kernel, whose epilogue forms the column sums (the 128-wide kernel leaves them to ia_colsum); asserted through
ia_gemm_dgrad_rows_filters.  Lengths 255 .. 1: groups with 4, 3, 2, 1 and 0 live blocks, groups that straddle two sequences."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
B, L = 10, 255
LENS = (255, 40, 130, 1, 200, 70, 255, 97, 33, 180)


def randn(shape, seed, dev, scale=1.0):
    return (torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale).to(dev)


def stream():
    return torch.cuda.current_stream().cuda_stream


def key_mask(dev, lens=LENS, length=L):
    return (torch.arange(length)[None] < torch.tensor(lens)[:, None]).to(torch.uint8).to(dev).contiguous()


def block_rows(live):
    """rows of the 32-row blocks that hold a live row"""
    M = live.numel()
    v = torch.cat((live, live.new_zeros((-M) % 32))).view(-1, 32)
    return v.any(dim=1, keepdim=True).expand_as(v).reshape(-1)[:M]


def device_list(lib, live):
    M = live.numel()
    out = torch.full((lib.ia_row_groups_packed_bytes(M) // 4,), -7, device=live.device, dtype=torch.int32)
    from item_alignment_amd import _lib
    _lib.check(lib.ia_row_groups_packed(live.data_ptr(), M, out.data_ptr(), stream()), "ia_row_groups_packed")
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("case", ["ragged", "bench_like", "all_dead", "all_live"])
def test_device_list_equals_host_list(gpu, case):
    from item_alignment_amd import _lib
    lib = _lib.load()
    if case == "ragged":
        live = key_mask(gpu).view(-1)
    elif case == "bench_like":
        rs = np.random.RandomState(0)
        lens = 3 + rs.randint(8, 49, size=512) + rs.randint(16, 204, size=512)
        lens[0] = 255
        live = key_mask(gpu, lens.tolist(), 255).view(-1)
    else:
        live = torch.full((B * L,), 0 if case == "all_dead" else 1, device=gpu, dtype=torch.uint8)
    M = live.numel()
    dev = device_list(lib, live).cpu().numpy()
    host = np.full(dev.size, -7, np.int32)
    live_np = np.ascontiguousarray(live.cpu().numpy())
    assert lib.ia_row_groups_packed_host(live_np.ctypes.data, M, host.ctypes.data) == 0
    nb = (M + 31) // 32
    nbr = (nb + 7) & ~7
    n_slots, n_dead = int(host[0]), int(host[1])
    assert (dev[:8] == host[:8]).all()
    assert (dev[8:8 + n_slots] == host[8:8 + n_slots]).all()
    assert (dev[8 + nbr:8 + nbr + n_dead] == host[8 + nbr:8 + nbr + n_dead]).all()


@pytest.mark.parametrize("shadow", [1, 0])
def test_packed_dgelu_colsum_equals_dense(gpu, shadow):
    """dX = (dY W) * aux and C2 += column sums.  aux is NaN in the blocks without a live row (not fetched), dX is NaN-poisoned beforehand."""
    from item_alignment_amd import _lib
    lib = _lib.load()
    M, N, K = B * L, 4096, 128
    assert lib.ia_gemm_dgrad_rows_filters(M, N, K) == 1
    live = key_mask(gpu).view(-1)
    lv, blk = live.bool(), block_rows(live.bool())
    assert 0 < blk.sum().item() < M
    dY = (randn((M, K), 5, gpu) * live[:, None]).to(BF).contiguous()                # zero on the dead rows: the contract
    W = randn((K, N), 6, gpu, 0.05).to(BF)                                           # the Linear's weight [K_out, N_in]
    Wt = W.t().contiguous()
    aux = randn((M, N), 7, gpu).to(BF)
    w_ptr, w_ks, ldw = (Wt.data_ptr(), 0, K) if shadow else (W.data_ptr(), 1, N)
    ws_bytes = lib.ia_gemm_colsum_workspace_bytes(M, N)
    c2_ref, c2 = randn((N,), 8, gpu), randn((N,), 8, gpu)                            # both accumulate on top of the same values
    ref = torch.empty((M, N), device=gpu, dtype=BF)
    ws = torch.full((ws_bytes,), 0xFF, device=gpu, dtype=torch.uint8)
    _lib.check(lib.ia_gemm_bf16(dY.data_ptr(), 0, K, w_ptr, w_ks, ldw, ref.data_ptr(), 0, N, M, N, K, 6, None, aux.data_ptr(), N, c2_ref.data_ptr(), 0,
                                ws.data_ptr(), ws_bytes, stream()), "dense")
    plist = device_list(lib, live)
    out = torch.full((M, N), float("nan"), device=gpu, dtype=BF)
    ws2 = torch.full((ws_bytes,), 0xFF, device=gpu, dtype=torch.uint8)
    auxp = aux.clone()
    auxp[~blk] = float("nan")
    _lib.check(lib.ia_gemm_dgrad_packed(dY.data_ptr(), K, w_ptr, w_ks, ldw, out.data_ptr(), N, M, N, K, auxp.data_ptr(), N, c2.data_ptr(), plist.data_ptr(),
                                        ws2.data_ptr(), ws_bytes, stream()), "packed")
    torch.cuda.synchronize()
    assert torch.isfinite(ref.float()).all() and ref[lv].float().abs().max().item() > 0
    assert torch.isfinite(out.float()).all()
    assert out[~blk].float().abs().max().item() == 0.0                               # the fill: dead blocks' rows are zeros
    assert torch.equal(out, ref)
    assert torch.isfinite(c2).all() and not torch.equal(c2_ref, randn((N,), 8, gpu))
    assert torch.equal(c2, c2_ref)                                                   # the fc1 bias gradient, bit for bit


def test_layer_backward_with_packed_dgelu_equals_every_row(gpu):
    """ia_layer_bwd2 (post-LN, masked_rows_dead = 3) with the data gradients' lists withheld (ia_debug_dgrad_rows(0): every row) against the
    filtered call -- the packed list built per call, and handed in (ia_layer_cfg::key_rows.packed).  Every gradient is equal."""
    from item_alignment_amd import _lib
    from item_alignment_amd._lib import LayerCfg, LayerGrads, LayerWeights
    from test_engine_gpu import make_layer
    lib = _lib.load()
    H, I, NH, M = 128, 4096, 2, B * L
    assert lib.ia_gemm_dgrad_rows_filters(M, I, H) == 1
    P32 = make_layer(H, I, gpu, 3)
    mats = ("w_qkv", "w_o", "w_fc1", "w_fc2")
    Pb = {k: v.to(BF) for k, v in P32.items() if k in mats}
    Pt = {k: v.t().contiguous() for k, v in Pb.items()}
    w = LayerWeights()
    for k in P32:
        setattr(w, k, (Pb[k] if k in mats else P32[k]).data_ptr())
    for k in mats:
        setattr(w, "wt_" + k[2:], Pt[k].data_ptr())
    x = randn((M, H), 5, gpu).to(BF)
    mask = key_mask(gpu)
    live = mask.view(-1)
    dy = (randn((M, H), 6, gpu) * live[:, None]).to(BF).contiguous()                  # zero at the masked positions: the contract
    base = dict(B=B, L=L, H=H, I=I, nh=NH, pre_ln=0, eps=1e-12, hidden_drop=0.1, attn_drop=0.1, seed=11, layer_id=2, masked_rows_dead=3)
    st = stream()
    # the caller's lists: ia_row_blocks and the packed list, each in a tensor of its own
    blocks = torch.zeros(lib.ia_row_blocks_bytes(M), device=gpu, dtype=torch.uint8)
    packed = torch.zeros(lib.ia_row_groups_packed_bytes(M), device=gpu, dtype=torch.uint8)
    _lib.check(lib.ia_row_blocks(live.data_ptr(), M, blocks.data_ptr(), st), "ia_row_blocks")
    _lib.check(lib.ia_row_groups_packed(live.data_ptr(), M, packed.data_ptr(), st), "ia_row_groups_packed")

    def step(handed):
        cfg = LayerCfg(**base)
        if handed:
            cfg.key_rows.blocks, cfg.key_rows.packed = blocks.data_ptr(), packed.data_ptr()
        stash = torch.full((lib.ia_layer_stash_bytes(C.byref(cfg)),), 0xFF, device=gpu, dtype=torch.uint8)
        y = torch.zeros((M, H), device=gpu, dtype=BF)
        _lib.check(lib.ia_layer_fwd(C.byref(cfg), C.byref(w), x.data_ptr(), mask.data_ptr(), y.data_ptr(), stash.data_ptr(), st), "fwd")
        scratch = torch.full((lib.ia_layer_bwd_scratch_bytes(C.byref(cfg)),), 0xFF, device=gpu, dtype=torch.uint8)
        G = {k: torch.zeros_like(v) for k, v in P32.items()}
        g = LayerGrads()
        for k in P32:
            setattr(g, k, G[k].data_ptr())
        dx, dx2 = torch.full_like(dy, float("nan")), torch.full_like(dy, float("nan"))
        _lib.check(lib.ia_layer_bwd2(C.byref(cfg), C.byref(w), C.byref(g), x.data_ptr(), mask.data_ptr(), y.data_ptr(), stash.data_ptr(), dy.data_ptr(),
                                     None, dx.data_ptr(), dx2.data_ptr(), scratch.data_ptr(), scratch.numel(), st), "bwd2")
        torch.cuda.synchronize()
        return dict(dx=dx, dx2=dx2, G=G)
    was = lib.ia_debug_dgrad_rows(0)
    try:
        d = step(False)
    finally:
        lib.ia_debug_dgrad_rows(was)
    assert was == 1
    for handed in (False, True):
        f = step(handed)
        for name in ("dx", "dx2"):
            assert torch.isfinite(f[name].float()).all(), name
            assert d[name].float().abs().max().item() > 0, name
            assert torch.equal(f[name], d[name]), (name, handed)
        for k in P32:
            assert torch.isfinite(f["G"][k]).all(), k
            assert d["G"][k].abs().max().item() > 0.0, k
            assert torch.equal(f["G"][k], d["G"][k]), (k, handed)
