"""The query-row limit of the attention (ia_attn_fwd_q_rows / ia_attn_bwd_bias_q_rows, ia_layer_cfg::out_q_rows): under a head that reads
position 0 of each sequence only, the last layer's attention computes the query blocks in front of the limit and nothing else -- and every
value the caller can observe stays what the unlimited call gives, bit for bit (torch.equal).

1. the kernels through the C ABI, limited against unlimited on a d_out that is zero at positions >= n: the one-kernel backward (L = 255 and
   70, ragged masks, dropout on and off, limits inside the first / second / third 32-query block) and the dQ + dK/dV pair (L = 577 without
   a mask, L = 300 with one and dropout).  out / lse2 / dq / dk / dv / workspace of the limited call start as 0xFF bytes (NaN).
2. one layer, post-LN and pre-LN, with the row-0 out_row_live, with and without out_q_rows = 1, the stash poisoned.
3. a small CoCaForItemAlignment (sum, cls) step with ia_debug_q_rows on and off."""
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu
BF = torch.bfloat16


def randn(shape, seed, dev, scale=1.0):
    return (torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale).to(dev)


def stream():
    return torch.cuda.current_stream().cuda_stream


def length_mask(B, L, lens, dev):
    if lens is None:
        return None
    assert len(lens) == B and max(lens) == L
    return (torch.arange(L)[None] < torch.tensor(lens)[:, None]).to(torch.uint8).to(dev).contiguous()


def poisoned(shape, dev, dtype):
    """0xFF bytes (NaN as bf16 / fp32); the last dimension of `shape` counts bytes"""
    t = torch.full(shape, 0xFF, device=dev, dtype=torch.uint8)
    return t if dtype == torch.uint8 else t.view(dtype)


# ------------------------------------------------------------------------------------------------------------------- 1. kernels
FUSED = [(3, 2, 255, (255, 140, 27), drop, n) for drop in (0.1, 0.0) for n in (1, 33, 65)] + [(3, 2, 70, (70, 33, 5), 0.0, 1)]
PAIR = [(2, 2, 577, None, 0.0, 1), (2, 2, 577, None, 0.0, 130), (2, 2, 300, (300, 150), 0.1, 1)]


@pytest.mark.parametrize("B,nh,L,lens,drop,n", FUSED + PAIR)
def test_limited_attention_equals_unlimited(gpu, B, nh, L, lens, drop, n):
    from item_alignment_amd import _lib
    lib = _lib.load()
    H, M = nh * 64, B * L
    qkv = randn((M, 3 * H), 1, gpu).to(BF)
    mask = length_mask(B, L, lens, gpu)
    mp = None if mask is None else mask.data_ptr()
    pos = torch.arange(L, device=gpu).repeat(B)
    keep = pos < n                                                   # the contract: d_out is zero at positions >= n ...
    flags = 0
    if mask is not None and drop > 0:                                # ... and, with IA_ATTN_MASKED_ROWS_DEAD, at masked positions
        flags = 2
        keep = keep & mask.view(-1).bool()
    d_out = (randn((M, H), 2, gpu) * keep[:, None]).to(BF).contiguous()
    base = qkv.data_ptr()
    ws_bytes = lib.ia_attn_bwd_bias_workspace_bytes(B, nh, L)
    scale, seed = 0.125, 1234

    def run(q_rows):
        lim = q_rows > 0
        out = poisoned((M, H * 2), gpu, BF) if lim else torch.zeros((M, H), device=gpu, dtype=BF)
        lse = poisoned((B * nh * L * 4,), gpu, torch.float32) if lim else torch.zeros(B * nh * L, device=gpu)
        _lib.check(lib.ia_attn_fwd_q_rows(0, base, base + 2 * H, base + 4 * H, 3 * H, mp, out.data_ptr(), H, lse.data_ptr(), B, nh, L, scale, drop,
                                          seed, q_rows, stream()), "fwd")
        dqkv = poisoned((M, 3 * H * 2), gpu, BF)
        delta = poisoned((B * nh * L * 4,), gpu, torch.float32)
        ws = poisoned((ws_bytes,), gpu, torch.uint8)
        dbias = randn((3 * H,), 3, gpu)                              # accumulated into: both calls start from the same values
        g = dqkv.data_ptr()
        _lib.check(lib.ia_attn_bwd_bias_q_rows(flags, base, base + 2 * H, base + 4 * H, 3 * H, mp, out.data_ptr(), d_out.data_ptr(), H, lse.data_ptr(),
                                               delta.data_ptr(), g, g + 2 * H, g + 4 * H, 3 * H, dbias.data_ptr(), ws.data_ptr(), ws_bytes, B, nh, L,
                                               scale, drop, seed, q_rows, stream()), "bwd")
        torch.cuda.synchronize()
        return out, lse.view(B, nh, L), dqkv, dbias
    o_d, l_d, g_d, b_d = run(0)
    o_l, l_l, g_l, b_l = run(n)
    rows = pos < n
    assert torch.isfinite(o_l.float()).all()                         # every row of the limited call's output is finite
    assert o_d[rows].float().abs().max().item() > 0
    assert torch.equal(o_l[rows], o_d[rows])
    assert torch.equal(l_l[:, :, :n], l_d[:, :, :n])
    assert torch.isfinite(g_d.float()).all() and torch.isfinite(g_l.float()).all()
    for name, lo in (("dq", 0), ("dk", H), ("dv", 2 * H)):
        assert g_d[:, lo:lo + H].float().abs().max().item() > 0, name
        assert torch.equal(g_l[:, lo:lo + H], g_d[:, lo:lo + H]), name
    assert torch.isfinite(b_l).all() and not torch.equal(b_d, randn((3 * H,), 3, gpu))
    assert torch.equal(b_l, b_d)


# --------------------------------------------------------------------------------------------------------------------- 2. one layer
@pytest.mark.parametrize("pre_ln,B,L,lens", [(0, 6, 70, (70, 1, 33, 5, 64, 40)), (1, 3, 577, None)])
def test_layer_with_out_q_rows_equals_layer_without(gpu, pre_ln, B, L, lens):
    from item_alignment_amd import _lib
    from item_alignment_amd._lib import LayerCfg, LayerGrads, LayerWeights
    from test_engine_gpu import make_layer
    lib = _lib.load()
    H, I, NH, M = 128, 256, 2, B * L
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
    mask = length_mask(B, L, lens, gpu)
    mp = None if mask is None else mask.data_ptr()
    live = torch.zeros(M, dtype=torch.uint8)
    live[::L] = 1
    live = live.to(gpu)
    lv = live.bool()
    dy = (randn((M, H), 6, gpu) * live[:, None]).to(BF).contiguous()
    drop = 0.0 if pre_ln else 0.1
    base = dict(B=B, L=L, H=H, I=I, nh=NH, pre_ln=pre_ln, eps=1e-6 if pre_ln else 1e-12, hidden_drop=drop, attn_drop=drop, seed=11, layer_id=2,
                masked_rows_dead=0 if pre_ln else 3)
    st = stream()

    def step(q_rows):
        cfg = LayerCfg(**base)
        cfg.out_row_live = live.data_ptr()
        cfg.out_q_rows = q_rows
        stash = torch.full((lib.ia_layer_stash_bytes(C.byref(cfg)),), 0xFF, device=gpu, dtype=torch.uint8)
        y = torch.zeros((M, H), device=gpu, dtype=BF)
        _lib.check(lib.ia_layer_fwd(C.byref(cfg), C.byref(w), x.data_ptr(), mp, y.data_ptr(), stash.data_ptr(), st), "fwd")
        scratch = torch.full((lib.ia_layer_bwd_scratch_bytes(C.byref(cfg)),), 0xFF, device=gpu, dtype=torch.uint8)
        G = {k: torch.zeros_like(v) for k, v in P32.items()}
        g = LayerGrads()
        for k in P32:
            setattr(g, k, G[k].data_ptr())
        dx = torch.full_like(dy, float("nan"))
        dx2 = None if pre_ln else torch.full_like(dy, float("nan"))
        _lib.check(lib.ia_layer_bwd2(C.byref(cfg), C.byref(w), C.byref(g), x.data_ptr(), mp, y.data_ptr(), stash.data_ptr(), dy.data_ptr(), None,
                                     dx.data_ptr(), None if dx2 is None else dx2.data_ptr(), scratch.data_ptr(), scratch.numel(), st), "bwd2")
        torch.cuda.synchronize()
        return dict(y=y, dx=dx, dx2=dx2, G=G)
    d, f = step(0), step(1)
    assert torch.isfinite(f["y"][lv].float()).all() and d["y"][lv].float().abs().max().item() > 0
    assert torch.equal(f["y"][lv], d["y"][lv])
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
    # the switch: with it off the cfg with the limit is the cfg without
    was = lib.ia_debug_q_rows(0)
    try:
        h = step(1)
    finally:
        lib.ia_debug_q_rows(was)
    assert was == 1 and torch.equal(h["dx"], d["dx"]) and torch.equal(h["y"][lv], d["y"][lv])


# ----------------------------------------------------------------------------------------------------------------------- 3. the model
def test_coca_sum_step_with_q_rows_equals_step_without(gpu):
    import item_alignment_amd.models as M
    from bench import roberta_large_config
    from item_alignment_amd import _lib
    from item_alignment_amd.data.synthetic import SyntheticCocaPairs
    from item_alignment_amd.models import functional as Fn
    lib = _lib.load()
    cfg = roberta_large_config(hidden_size=128, num_hidden_layers=2, num_attention_heads=2, intermediate_size=512, vocab_size=21128,
                               image_size=128, max_seq_len=20, max_seq_len_pv=50)
    torch.manual_seed(0)
    text = M.RobertaModel(cfg)
    vit = M.VisionTransformer(img_size=128, patch_size=16, embed_dim=192, depth=2, num_heads=3)
    model = M.CoCaForItemAlignment(cfg, vit, text).cuda()
    model.ensure_arena()
    assert model.reads_cls_only()
    data = SyntheticCocaPairs(4, image_size=128, max_title=20, max_pv=50, seed=1)
    batch = data.batch([0, 1, 2, 3], "cuda")
    seen = []
    orig = text.encoder.layer_cfg

    def layer_cfg(*a, **k):
        c = orig(*a, **k)
        seen.append(c)
        return c

    def step(on):
        was = lib.ia_debug_q_rows(1 if on else 0)
        try:
            model.train()
            Fn.set_step_seed(77)
            torch.manual_seed(5)
            model.param_arena.zero_grad()
            out = model(*batch[:10], labels=batch[10])
            out.loss.backward()
            grads = {n: p.grad.detach().clone() for n, p in model.named_parameters() if p.grad is not None}
            torch.cuda.synchronize()
        finally:
            lib.ia_debug_q_rows(was)
        return out, grads
    text.encoder.__dict__["layer_cfg"] = layer_cfg
    try:
        on = step(True)
    finally:
        text.encoder.__dict__.pop("layer_cfg")
    assert [c.out_q_rows for c in seen] == [0, 1] and seen[1].L > 32      # the last layer carries the limit, no other layer does
    off = step(False)
    for k in ("loss", "logits", "probs"):
        a, b = getattr(on[0], k), getattr(off[0], k)
        assert torch.isfinite(a.float()).all(), k
        assert torch.equal(a, b), k
    assert on[1].keys() == off[1].keys() and len(on[1]) > 40
    for n in on[1]:
        assert torch.isfinite(on[1][n]).all(), n
        assert torch.equal(on[1][n], off[1][n]), n
    assert sum(1 for v in on[1].values() if v.abs().max().item() > 0) > 40
