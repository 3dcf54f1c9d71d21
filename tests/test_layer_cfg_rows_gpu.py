"""ia_layer_cfg::key_rows (ia_row_lists): every list is a pointer of its own, and masked_rows_dead holds the two promises and nothing else.

1. One post-LN layer under masked_rows_dead = 3 at the shape of tests/test_engine_slabs_gpu.py whose GEMMs all filter (B = 40, L = 255,
H = 1024, nh = 16, I = 1024: the slab kernels run, asserted), dropout on, fixed seed.  The five lists of the key mask come from the public
builders in FIVE separately allocated tensors, allocated in a shuffled order with a spacer full of 0xFF between every two of them: no
list can be found from another one's address.  Forward and backward with all five handed in, and with the slab list alone, are
torch.equal to the call with every pointer NULL (the layer builds its own): y, dx, dx2 and every parameter gradient.  Stash and scratch
are filled with 0xFF before each call.

2. A bit of masked_rows_dead other than the two promises (a caller written for the layout bits of ABI 20) is an argument error: the size
functions return 0 and ia_layer_fwd returns IA_ERR_ARG before anything is launched."""
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu

BUILDERS = {"blocks": "row_blocks", "packed": "row_groups_packed", "slabs": "row_slabs", "groups": "row_groups", "kblocks": "kblock_mask"}


def separate_lists(lib, mask, M, gpu, st):
    """the five lists of ia_row_lists, each in a tensor of its own; returns ({member: tensor}, the spacers)"""
    from item_alignment_amd import _lib
    lists, spacers = {}, []
    for member in ("slabs", "kblocks", "blocks", "groups", "packed"):      # (not the order of the struct, nor of any layer call's carve)
        name = BUILDERS[member]
        spacers.append(torch.full((4096 + 256 * len(spacers),), 0xFF, device=gpu, dtype=torch.uint8))
        lists[member] = torch.full((getattr(lib, f"ia_{name}_bytes")(M),), 0xFF, device=gpu, dtype=torch.uint8)
        _lib.check(getattr(lib, f"ia_{name}")(mask.data_ptr(), M, lists[member].data_ptr(), st), f"ia_{name}")
    spacers.append(torch.full((4096,), 0xFF, device=gpu, dtype=torch.uint8))
    ptrs = sorted(t.data_ptr() for t in lists.values())
    assert len(set(ptrs)) == 5
    return lists, spacers


def test_separately_allocated_lists_equal_the_layers_own(gpu):
    from item_alignment_amd import _lib
    from item_alignment_amd._lib import LayerCfg, LayerGrads, LayerWeights
    from test_engine_gpu import make_layer
    lib = _lib.load()
    B, L, H, NH, I = 40, 255, 1024, 16, 1024
    M = B * L
    assert [lib.ia_gemm_fwd_rows_filters(M, n, k) for n, k in ((3 * H, H), (H, H), (I, H), (H, I))] == [1, 1, 1, 1]
    assert [lib.ia_gemm_dgrad_rows_filters(M, n, k) for n, k in ((H, I), (H, H), (H, 3 * H))] == [1, 1, 1]
    P32 = make_layer(H, I, gpu, 3)
    mats = ("w_qkv", "w_o", "w_fc1", "w_fc2")
    Pb = {k: v.to(torch.bfloat16) for k, v in P32.items() if k in mats}
    Pt = {k: v.t().contiguous() for k, v in Pb.items()}
    w = LayerWeights()
    for k in P32:
        setattr(w, k, (Pb[k] if k in mats else P32[k]).data_ptr())
    for k in mats:
        setattr(w, "wt_" + k[2:], Pt[k].data_ptr())
    x = torch.randn(M, H, generator=torch.Generator().manual_seed(5)).to(gpu).to(torch.bfloat16)
    ragged = [L, 1, 27, 130, 200, 9, 101, 33, 180, 64]                       # one sequence of full length, one of length 1
    lens = torch.tensor([ragged[i % len(ragged)] for i in range(B)])
    mask = (torch.arange(L)[None] < lens[:, None]).to(torch.uint8).to(gpu).contiguous()
    valid = mask.bool().view(-1)
    dy = torch.randn(M, H, generator=torch.Generator().manual_seed(6)).to(gpu).to(torch.bfloat16)
    dy = (dy * valid[:, None].to(dy.dtype)).contiguous()          # zero at masked positions: what masked_rows_dead promises
    st = torch.cuda.current_stream().cuda_stream
    lists, spacers = separate_lists(lib, mask, M, gpu, st)

    def step(given):
        cfg = LayerCfg(B=B, L=L, H=H, I=I, nh=NH, pre_ln=0, eps=1e-12, hidden_drop=0.1, attn_drop=0.1, seed=11, layer_id=2, masked_rows_dead=3)
        for member in given:
            setattr(cfg.key_rows, member, lists[member].data_ptr())
        assert [getattr(cfg.key_rows, m) is not None for m in BUILDERS] == [m in given for m in BUILDERS]
        stash = torch.full((lib.ia_layer_stash_bytes(C.byref(cfg)),), 0xFF, device=gpu, dtype=torch.uint8)
        y = torch.full((M, H), -1, device=gpu, dtype=torch.int16).view(torch.bfloat16)
        _lib.check(lib.ia_layer_fwd(C.byref(cfg), C.byref(w), x.data_ptr(), mask.data_ptr(), y.data_ptr(), stash.data_ptr(), st), f"fwd {given}")
        scratch = torch.full((lib.ia_layer_bwd_scratch_bytes(C.byref(cfg)),), 0xFF, device=gpu, dtype=torch.uint8)
        G = {k: torch.zeros_like(v) for k, v in P32.items()}
        g = LayerGrads()
        for k in P32:
            setattr(g, k, G[k].data_ptr())
        dx, dx2 = torch.full_like(dy, float("nan")), torch.full_like(dy, float("nan"))
        _lib.check(lib.ia_layer_bwd2(C.byref(cfg), C.byref(w), C.byref(g), x.data_ptr(), mask.data_ptr(), y.data_ptr(), stash.data_ptr(), dy.data_ptr(),
                                     None, dx.data_ptr(), dx2.data_ptr(), scratch.data_ptr(), scratch.numel(), st), f"bwd2 {given}")
        torch.cuda.synchronize()
        return dict(y=y, dx=dx, dx2=dx2, **G)

    own = step(())
    assert own["y"][valid].float().abs().max().item() > 0 and own["y"][~valid].float().abs().max().item() == 0.0
    for given in (tuple(BUILDERS), ("slabs",)):
        got = step(given)
        for name in own:
            assert torch.isfinite(got[name].float()).all(), (name, given)
            assert own[name].float().abs().max().item() > 0, name
            assert torch.equal(got[name], own[name]), (name, given)
    assert all(bool((s == 0xFF).all()) for s in spacers)              # nothing was written, or built, next to a list


def test_unknown_promise_bit_is_refused(gpu):
    from item_alignment_amd import _lib
    from item_alignment_amd._lib import LayerCfg, LayerWeights
    lib = _lib.load()
    B, L, H, NH, I = 2, 16, 128, 2, 256
    base = dict(B=B, L=L, H=H, I=I, nh=NH, pre_ln=0, eps=1e-12, hidden_drop=0.0, attn_drop=0.0, seed=1, layer_id=0)
    good, stale = LayerCfg(masked_rows_dead=3, **base), LayerCfg(masked_rows_dead=3 | 4, **base)
    sizes = (lib.ia_layer_stash_bytes, lib.ia_layer_bwd_scratch_bytes, lib.ia_layer_infer_scratch_bytes)
    assert all(fn(C.byref(good)) > 0 for fn in sizes)
    assert [fn(C.byref(stale)) for fn in sizes] == [0, 0, 0]
    x = torch.zeros(B * L, H, device=gpu, dtype=torch.bfloat16)
    y = torch.zeros_like(x)
    stash = torch.zeros(lib.ia_layer_stash_bytes(C.byref(good)), device=gpu, dtype=torch.uint8)
    mask = torch.ones(B, L, device=gpu, dtype=torch.uint8)
    w = LayerWeights()                                              # (never read: the cfg is refused first)
    st = torch.cuda.current_stream().cuda_stream
    rc = lib.ia_layer_fwd(C.byref(stale), C.byref(w), x.data_ptr(), mask.data_ptr(), y.data_ptr(), stash.data_ptr(), st)
    assert rc == -1 and lib.ia_strerror(rc).decode().startswith("invalid argument")
