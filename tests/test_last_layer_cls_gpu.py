"""ia_layer_cfg::out_row_live (ABI 20): the part of an encoder layer behind its attention computed for the rows the head reads only --
row 0 of each sequence -- and everything the caller can observe stays what the every-row call gives, bit for bit (torch.equal).

Shapes: the smallest at which every GEMM of the layer reaches the 256-wide kernels, whose remapped forms do the filtering (asserted through
the *_filters queries): ViT-like B = 24, L = 577 (M = 13 848), H = 768, nh = 12, I = 3072, pre-LN; text-like B = 41, L = 255 (M = 10 455, no
multiple of 128), H = 1024, nh = 16, I = 4096, post-LN, a ragged key mask with one sequence of length 1 and one of 255, dropout 0.1.

1. the kernels through the C ABI: the remapped IA_EPI_BIAS_ADD GEMM, the group-aligned x gelu' + column-sums GEMM, the row-filtered
   LayerNorm backward in the pre-LN block's form (dres) and the final norm's form;
2. one layer, pre-LN and post-LN: ia_layer_fwd + ia_layer_fwd_infer + ia_layer_bwd2 with out_row_live against the same calls without it,
   stash, scratch and y filled with 0xFF (NaN) in front of the filtered calls;
3. a two-layer-per-tower CoCaForItemAlignment (sum) step with the rows skipped against ia_debug_out_rows(0), and who opts in."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

VIT = dict(B=24, L=577, H=768, NH=12, I=3072, pre_ln=1)
TXT = dict(B=41, L=255, H=1024, NH=16, I=4096, pre_ln=0)
BF = torch.bfloat16


def randn(shape, seed, dev, scale=1.0):
    return (torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale).to(dev)


def cls_live(B, L, dev, extra_last=False):
    m = torch.zeros(B * L, dtype=torch.uint8)
    m[::L] = 1
    if extra_last:
        m[-1] = 1
    return m.to(dev)


def dilate(live, unit):
    """rows of the `unit`-row blocks that hold a live row"""
    M = live.numel()
    pad = (-M) % unit
    v = torch.cat((live, live.new_zeros(pad))).view(-1, unit)
    return v.any(dim=1, keepdim=True).expand_as(v).reshape(-1)[:M]


def nan_fill(t, rows):
    t = t.clone()
    t[rows] = float("nan")
    return t


def stream():
    return torch.cuda.current_stream().cuda_stream


# ------------------------------------------------------------------------------------------------------------------- 1. kernels
@pytest.mark.parametrize("fill", [0, 1])
def test_bias_add_gemm_over_live_blocks_equals_dense(gpu, fill):
    """the ViT fc2: Y = X W^T + bias + aux.  Rows of X and aux in blocks without a live row are NaN: they are not fetched."""
    from item_alignment_amd import _lib
    lib = _lib.load()
    M, N, K = VIT["B"] * VIT["L"], VIT["H"], VIT["I"]
    assert lib.ia_gemm_fwd_rows_filters(M, N, K) == 1
    live = cls_live(VIT["B"], VIT["L"], gpu)
    blk = dilate(live.bool(), 32)
    assert 0 < blk.sum().item() < M
    X, W = randn((M, K), 1, gpu).to(BF), randn((N, K), 2, gpu, 0.05).to(BF)
    aux, bias = randn((M, N), 3, gpu).to(BF), randn((N,), 4, gpu, 0.1)
    ref = torch.empty((M, N), device=gpu, dtype=BF)
    _lib.check(lib.ia_gemm_bf16(X.data_ptr(), 0, K, W.data_ptr(), 0, K, ref.data_ptr(), 0, N, M, N, K, 5, bias.data_ptr(), aux.data_ptr(), N, None, 0,
                                None, 0, stream()), "dense")
    Xp, auxp = nan_fill(X, ~blk), nan_fill(aux, ~blk)
    out = torch.full((M, N), 7.0, device=gpu, dtype=BF)
    ws = torch.empty(lib.ia_gemm_fwd_rows_workspace_bytes(M), device=gpu, dtype=torch.uint8)
    _lib.check(lib.ia_gemm_fwd_rows_add(Xp.data_ptr(), K, W.data_ptr(), K, out.data_ptr(), N, M, N, K, bias.data_ptr(), auxp.data_ptr(), N,
                                        live.data_ptr(), fill, ws.data_ptr(), ws.numel(), stream()), "filtered")
    torch.cuda.synchronize()
    assert torch.isfinite(ref.float()).all() and ref.float().abs().max().item() > 0
    assert torch.equal(out[blk], ref[blk])
    assert torch.equal(out[~blk], torch.full_like(out[~blk], 0.0 if fill else 7.0))


@pytest.mark.parametrize("shape,shadow,extra_last", [("vit", 0, False), ("vit", 1, False), ("txt", 1, False), ("txt", 0, True)])
def test_dgelu_colsum_gemm_over_live_groups_equals_dense(gpu, shape, shadow, extra_last):
    """dX = (dY W) * aux and C2 += column sums: whole 128-row groups, the fc1 bias gradient bit for bit.  aux is NaN in the groups left out."""
    from item_alignment_amd import _lib
    lib = _lib.load()
    s = VIT if shape == "vit" else TXT
    M, N, K = s["B"] * s["L"], s["I"], s["H"]
    assert lib.ia_gemm_dgrad_rows_filters(M, N, K) == 1
    live = cls_live(s["B"], s["L"], gpu, extra_last)
    grp = dilate(live.bool(), 128)
    assert 0 < grp.sum().item() < M
    dY = (randn((M, K), 5, gpu) * live[:, None]).to(BF).contiguous()                # zero outside the live rows: the contract
    W = randn((K, N), 6, gpu, 0.05).to(BF)                                           # the Linear's weight [K_out, N_in]
    Wt = W.t().contiguous()
    aux = randn((M, N), 7, gpu).to(BF)
    w_ptr, w_ks, ldw = (Wt.data_ptr(), 0, K) if shadow else (W.data_ptr(), 1, N)
    ws_bytes = lib.ia_gemm_dgrad_rows_workspace_bytes(M, N, K)
    c2_ref, c2 = randn((N,), 8, gpu), randn((N,), 8, gpu)                            # both accumulate on top of the same values
    ref = torch.empty((M, N), device=gpu, dtype=BF)
    ws = torch.full((ws_bytes,), 0xFF, device=gpu, dtype=torch.uint8)
    _lib.check(lib.ia_gemm_bf16(dY.data_ptr(), 0, K, w_ptr, w_ks, ldw, ref.data_ptr(), 0, N, M, N, K, 6, None, aux.data_ptr(), N, c2_ref.data_ptr(), 0,
                                ws.data_ptr(), ws_bytes, stream()), "dense")
    out = torch.full((M, N), 7.0, device=gpu, dtype=BF)
    ws2 = torch.full((ws_bytes,), 0xFF, device=gpu, dtype=torch.uint8)
    auxp = nan_fill(aux, ~grp)
    _lib.check(lib.ia_gemm_dgrad_groups_rows(dY.data_ptr(), K, w_ptr, w_ks, ldw, out.data_ptr(), N, M, N, K, auxp.data_ptr(), N, c2.data_ptr(),
                                             live.data_ptr(), ws2.data_ptr(), ws_bytes, stream()), "grouped")
    torch.cuda.synchronize()
    assert ref[live.bool()].float().abs().max().item() > 0
    assert torch.equal(out[grp], ref[grp])
    assert out[~grp].float().abs().max().item() == 0.0
    assert torch.isfinite(c2).all() and not torch.equal(c2_ref, randn((N,), 8, gpu))
    assert torch.equal(c2, c2_ref)


@pytest.mark.parametrize("form", ["pre_ln_ln2", "final_norm"])
def test_ln_backward_over_live_rows_equals_dense(gpu, form):
    """ia_ln_bwd2_rows in the forms the ViT uses (dres = the residual gradient; none) against ia_ln_bwd: dz on the live rows, zeros elsewhere,
    and the gamma / beta / bias sums.  The dead rows of z, mean and rstd are NaN: they are not fetched."""
    from item_alignment_amd import _lib
    lib = _lib.load()
    M, H = VIT["B"] * VIT["L"], VIT["H"]
    live = cls_live(VIT["B"], VIT["L"], gpu)
    lv = live.bool()
    dy = (randn((M, H), 11, gpu) * live[:, None]).to(BF).contiguous()
    dres = (randn((M, H), 12, gpu) * live[:, None]).to(BF).contiguous() if form == "pre_ln_ln2" else None
    z = randn((M, H), 13, gpu).to(BF)
    mean, rstd = z.float().mean(1).contiguous(), (1.0 / (z.float().std(1) + 1e-3)).contiguous()
    gamma = 1 + randn((H,), 14, gpu, 0.1)
    ws_bytes = lib.ia_ln_bwd_workspace_bytes(M, H)

    def run(filtered):
        zz, mm, rr = (nan_fill(t, ~lv) for t in (z, mean, rstd)) if filtered else (z, mean, rstd)
        dz = torch.full((M, H), 7.0, device=gpu, dtype=BF)
        sums = [randn((H,), 15 + i, gpu) for i in range(3)]
        ws = torch.full((ws_bytes,), 0xFF, device=gpu, dtype=torch.uint8)
        dres_p = None if dres is None else dres.data_ptr()
        if filtered:
            rc = lib.ia_ln_bwd2_rows(dy.data_ptr(), None, dres_p, zz.data_ptr(), mm.data_ptr(), rr.data_ptr(), gamma.data_ptr(), dz.data_ptr(), None,
                                     sums[0].data_ptr(), sums[1].data_ptr(), sums[2].data_ptr(), M, H, 0.0, 0, 0, live.data_ptr(), ws.data_ptr(),
                                     ws_bytes, 1, stream())
        else:
            rc = lib.ia_ln_bwd(dy.data_ptr(), dres_p, zz.data_ptr(), mm.data_ptr(), rr.data_ptr(), gamma.data_ptr(), dz.data_ptr(), None,
                               sums[0].data_ptr(), sums[1].data_ptr(), sums[2].data_ptr(), M, H, 0.0, 0, 0, ws.data_ptr(), ws_bytes, 1, stream())
        _lib.check(rc, "ln backward")
        torch.cuda.synchronize()
        return dz, sums
    dz_d, s_d = run(False)
    dz_f, s_f = run(True)
    assert dz_d[lv].float().abs().max().item() > 0
    assert torch.equal(dz_f[lv], dz_d[lv])
    assert dz_f[~lv].float().abs().max().item() == 0.0 and dz_d[~lv].float().abs().max().item() == 0.0
    for a, b, name in zip(s_d, s_f, ("dgamma", "dbeta", "dbias")):
        assert torch.isfinite(b).all(), name
        assert torch.equal(a, b), name


# --------------------------------------------------------------------------------------------------------------------- 2. one layer
def text_mask(B, L, dev):
    lengths = [255, 1, 64, 27, 130, 200, 9, 101, 33, 180]
    lens = torch.tensor([min(L, lengths[i % len(lengths)]) for i in range(B)])
    assert lens.min().item() == 1 and lens.max().item() == L
    return (torch.arange(L)[None] < lens[:, None]).to(torch.uint8).to(dev).contiguous()


@pytest.mark.parametrize("shape,host_lists", [("vit", False), ("vit", True), ("txt", False), ("txt", True)])
def test_layer_with_out_row_live_equals_every_row_call(gpu, shape, host_lists):
    from item_alignment_amd import _lib
    from item_alignment_amd._lib import LayerCfg, LayerGrads, LayerWeights
    from test_engine_gpu import make_layer
    lib = _lib.load()
    s = VIT if shape == "vit" else TXT
    B, L, H, I, NH, pre_ln = s["B"], s["L"], s["H"], s["I"], s["NH"], s["pre_ln"]
    M = B * L
    # every GEMM of the layer takes the filtered kernels at this shape
    assert [lib.ia_gemm_fwd_rows_filters(M, n, k) for n, k in ((3 * H, H), (H, H), (I, H), (H, I))] == [1, 1, 1, 1]
    assert [lib.ia_gemm_dgrad_rows_filters(M, n, k) for n, k in ((I, H), (H, I), (H, H), (H, 3 * H))] == [1, 1, 1, 1]
    assert [lib.ia_gemm_wgrad_rows_filters(no, ni, M) for no, ni in ((H, I), (I, H), (H, H), (3 * H, H))] == [1, 1, 1, 1]
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
    mask = None if pre_ln else text_mask(B, L, gpu)
    live = cls_live(B, L, gpu)
    lv = live.bool()
    if mask is not None:
        assert mask.view(-1)[lv].all()                               # every out_row_live row is a live key
    dy = (randn((M, H), 6, gpu) * live[:, None]).to(BF).contiguous()                  # zero outside out_row_live: the contract
    drop = 0.0 if pre_ln else 0.1
    base = dict(B=B, L=L, H=H, I=I, nh=NH, pre_ln=pre_ln, eps=1e-6 if pre_ln else 1e-12, hidden_drop=drop, attn_drop=drop, seed=11, layer_id=2,
                masked_rows_dead=0 if pre_ln else 3)
    cfg_d, cfg_f = LayerCfg(**base), LayerCfg(**base)
    cfg_f.out_row_live = live.data_ptr()
    lists = None
    if host_lists:
        live_np = np.ascontiguousarray(live.cpu().numpy())
        rb, kb, rg = (np.zeros(n // 4, np.int32) for n in (lib.ia_row_blocks_bytes(M), lib.ia_kblock_mask_bytes(M), lib.ia_row_groups_bytes(M)))
        assert lib.ia_row_blocks_host(live_np.ctypes.data, M, rb.ctypes.data) == 0
        assert lib.ia_kblock_mask_host(live_np.ctypes.data, M, kb.ctypes.data) == 0
        assert lib.ia_row_groups_host(live_np.ctypes.data, M, rg.ctypes.data) == 0
        lists = [torch.from_numpy(a).to(gpu) for a in (rb, kb, rg)]
        cfg_f.out_rows.blocks, cfg_f.out_rows.kblocks, cfg_f.out_rows.groups = (t.data_ptr() for t in lists)
    mp = None if mask is None else mask.data_ptr()
    st = stream()

    def step(cfg, poison):
        fillv = 0xFF if poison else 0
        stash = torch.full((lib.ia_layer_stash_bytes(C.byref(cfg)),), fillv, device=gpu, dtype=torch.uint8)
        y = torch.full((M, H), -1 if poison else 0, device=gpu, dtype=torch.int16).view(BF)
        yi = torch.full((M, H), -1 if poison else 0, device=gpu, dtype=torch.int16).view(BF)
        isc = torch.full((lib.ia_layer_infer_scratch_bytes(C.byref(cfg)),), fillv, device=gpu, dtype=torch.uint8)
        _lib.check(lib.ia_layer_fwd(C.byref(cfg), C.byref(w), x.data_ptr(), mp, y.data_ptr(), stash.data_ptr(), st), "fwd")
        _lib.check(lib.ia_layer_fwd_infer(C.byref(cfg), C.byref(w), x.data_ptr(), mp, yi.data_ptr(), isc.data_ptr(), isc.numel(), st), "fwd_infer")
        scratch = torch.full((lib.ia_layer_bwd_scratch_bytes(C.byref(cfg)),), fillv, device=gpu, dtype=torch.uint8)
        G = {k: torch.zeros_like(v) for k, v in P32.items()}
        g = LayerGrads()
        for k in P32:
            setattr(g, k, G[k].data_ptr())
        colsum = torch.zeros(H, device=gpu)
        if pre_ln:
            cfg.dx_colsum_out = colsum.data_ptr()
        dx = torch.full_like(dy, float("nan"))
        dx2 = None if pre_ln else torch.full_like(dy, float("nan"))
        _lib.check(lib.ia_layer_bwd2(C.byref(cfg), C.byref(w), C.byref(g), x.data_ptr(), mp, y.data_ptr(), stash.data_ptr(), dy.data_ptr(), None,
                                     dx.data_ptr(), None if dx2 is None else dx2.data_ptr(), scratch.data_ptr(), scratch.numel(), st), "bwd2")
        torch.cuda.synchronize()
        return dict(y=y, yi=yi, dx=dx, dx2=dx2, G=G, colsum=colsum)
    d, f = step(cfg_d, False), step(cfg_f, True)
    for name in ("y", "yi"):
        assert torch.isfinite(d[name].float()).all() and d[name][lv].float().abs().max().item() > 0, name
        assert torch.equal(f[name][lv], d[name][lv]), name
    if not pre_ln:                                                   # a post-LN layer leaves zeros outside out_row_live
        assert f["y"][~lv].float().abs().max().item() == 0.0 and f["yi"][~lv].float().abs().max().item() == 0.0
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
    if pre_ln:
        assert d["colsum"].abs().max().item() > 0.0 and torch.equal(f["colsum"], d["colsum"])
    # the hook: with it off the filtered cfg is the every-row call (y is then written in every row)
    was = lib.ia_debug_out_rows(0)
    try:
        h = step(cfg_f, True)
    finally:
        lib.ia_debug_out_rows(was)
    assert torch.equal(h["y"], d["y"]) and torch.equal(h["dx"], d["dx"])
    del lists


# ----------------------------------------------------------------------------------------------------------------------- 3. the model
PAIRS = 21      # 42 sequences of 255 tokens and 42 images of 577 tokens: both towers' last layers reach the 256-wide kernels


@pytest.fixture(scope="module")
def coca_model(gpu):
    import item_alignment_amd.models as M
    from bench import roberta_large_config
    from item_alignment_amd.data.synthetic import SyntheticCocaPairs
    cfg = roberta_large_config(num_hidden_layers=2)
    torch.manual_seed(0)
    text = M.RobertaModel(cfg)
    vit = M.VisionTransformer(img_size=384, patch_size=16, embed_dim=768, depth=2, num_heads=12)
    model = M.CoCaForItemAlignment(cfg, vit, text).cuda()
    model.ensure_arena()
    data = SyntheticCocaPairs(PAIRS, image_size=384, max_title=50, max_pv=205, seed=1)
    batch = list(data.batch(list(range(PAIRS)), "cuda"))
    # one sequence of length 1 and one of full length among the ragged ones
    m1 = batch[1].clone()
    m1[0, 1:] = 0
    m1[1, :] = 1
    batch[1] = m1
    return model, cfg, batch


def record_cfgs(stack, seen):
    """keep every ia_layer_cfg the stack hands to the engine (EncoderStackFn fills the optional fields in afterwards)"""
    orig = stack.layer_cfg

    def layer_cfg(*a, **k):
        c = orig(*a, **k)
        seen.append(c)
        return c
    stack.__dict__["layer_cfg"] = layer_cfg
    return lambda: stack.__dict__.pop("layer_cfg")


def out_fields(c):
    return (c.out_row_live, c.out_rows.blocks, c.out_rows.kblocks, c.out_rows.groups)


def train_step(model, batch, on):
    from item_alignment_amd import _lib
    from item_alignment_amd.models import functional as Fn
    lib = _lib.load()
    seen_t, seen_v = [], []
    undo = [record_cfgs(model.coca.text_encoder.encoder, seen_t), record_cfgs(model.coca.img_encoder, seen_v)]
    was = lib.ia_debug_out_rows(1 if on else 0)
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
        lib.ia_debug_out_rows(was)
        for u in undo:
            u()
    return out, grads, seen_t, seen_v


def test_coca_sum_step_with_cls_rows_only_equals_every_row_step(coca_model):
    model, cfg, batch = coca_model
    on, off = train_step(model, batch, True), train_step(model, batch, False)
    for seen in (on[2], on[3]):                                      # the last layer of each tower carries the fields, no other layer does
        assert len(seen) == 2
        assert all(v is None for v in out_fields(seen[0])) and all(v is not None for v in out_fields(seen[1]))
    for k in ("loss", "logits", "probs", "src_embeds", "tgt_embeds"):
        a, b = getattr(on[0], k), getattr(off[0], k)
        assert torch.isfinite(a.float()).all(), k
        assert torch.equal(a, b), k
    assert on[1].keys() == off[1].keys() and len(on[1]) > 40
    for n in on[1]:
        assert torch.isfinite(on[1][n]).all(), n
        assert torch.equal(on[1][n], off[1][n]), n
    assert sum(1 for v in on[1].values() if v.abs().max().item() > 0) > 40


def test_only_the_cls_sum_head_opts_in(coca_model, monkeypatch):
    """every caller the issue lists as kept dense leaves the ABI 20 fields NULL in every layer's cfg"""
    from item_alignment_amd.models import text as text_mod
    model, cfg, batch = coca_model
    text, vit = model.coca.text_encoder, model.coca.img_encoder
    ids, mask, tts = batch[0], batch[1], batch[2]
    images = batch[4]

    def fields_of(call, stacks=(text.encoder, vit)):
        seen = []
        undo = [record_cfgs(s, seen) for s in stacks]
        try:
            with torch.no_grad():
                call()
            torch.cuda.synchronize()
        finally:
            for u in undo:
                u()
        assert seen
        return [out_fields(c) for c in seen]

    def all_null(call, stacks=(text.encoder, vit)):
        return all(v is None for f in fields_of(call, stacks) for v in f)
    model.eval()
    full = lambda: model(*batch[:10], labels=batch[10])
    assert not all_null(full)                                                                           # the one caller that opts in
    assert all_null(lambda: text(ids, attention_mask=mask, token_type_ids=tts))                         # a direct RobertaModel call
    assert all_null(lambda: text(ids, attention_mask=mask, token_type_ids=tts, padded_rows_unread=True))
    assert all_null(lambda: text(ids, attention_mask=mask, token_type_ids=tts, padded_rows_unread=True, cls_only_read=True,
                                 output_hidden_states=True))
    assert all_null(lambda: text(ids, attention_mask=mask, token_type_ids=tts, cls_only_read=True))     # not without padded_rows_unread
    assert not all_null(lambda: text(ids, attention_mask=mask, token_type_ids=tts, padded_rows_unread=True, cls_only_read=True))
    assert all_null(lambda: vit.forward_features(images))                                               # the default ViT call
    assert all_null(lambda: vit(images))
    assert not all_null(lambda: vit.forward_features(images, cls_only=True))
    assert all_null(lambda: model.coca.embed_text(ids, mask, tts, None))                                # CoCaModel passes nothing by itself
    assert all_null(lambda: model.coca.embed_text(ids, mask, tts, None, padded_rows_matter=True, cls_only_read=True))      # cross_attn's call
    assert all_null(lambda: model.coca.embed_image(images))
    assert model.reads_cls_only()
    for name, value in (("cls_layers", "1,2"), ("auxiliary_task", True)):      # the whole model under the changed config: four dense layers
        monkeypatch.setattr(cfg, name, value)
        assert not model.reads_cls_only(), name
        assert len(fields_of(full)) == 4 and all_null(full), name
        monkeypatch.undo()
    # vec_sim: the towers as the model's forward calls them, with the model's own decision
    monkeypatch.setattr(cfg, "classification_method", "vec_sim")
    assert not model.reads_cls_only()
    assert all_null(lambda: (model.coca.embed_image(images, cls_only=model.reads_cls_only()),
                             model.coca.embed_text(ids, mask, tts, None, cls_only_read=model.reads_cls_only())))
    monkeypatch.undo()
    monkeypatch.setattr(model, "ensemble", "cross_attn")
    assert not model.reads_cls_only()
    monkeypatch.undo()
    assert model.reads_cls_only() and not all_null(full)
    monkeypatch.setattr(text_mod, "UNPAD", True)                                                         # packed rows (cu_seqlens)
    assert all_null(full, stacks=(text.encoder,))
    monkeypatch.undo()


def test_pkgm_tower_keeps_every_row(gpu):
    """a PKGM model run: its text model never passes the flag, every layer's cfg keeps the ABI 20 fields NULL"""
    from golden_util import load_case
    from test_models_gpu import build, g
    case = load_case("pkgm_one_tower")
    model = build(case, "PKGMOneTower")
    seen = []
    undo = record_cfgs(model.roberta.encoder, seen)
    try:
        out = model(input_ids=g(case, "input_ids"), attention_mask=g(case, "attention_mask"), token_type_ids=g(case, "token_type_ids"),
                    position_ids=g(case, "position_ids"), labels=g(case, "labels"))
        torch.cuda.synchronize()
        assert torch.isfinite(out.loss).all()
    finally:
        undo()
    assert seen and all(v is None for c in seen for v in out_fields(c))


def test_masked_first_position_is_no_out_row(coca_model):
    """every out_row_live row is a live key by construction: a sequence whose position 0 is masked has no row behind the attention.  Its row 0
    of the last hidden state is the row of zeros the key-mask filter leaves, it passes no gradient, and the step equals the every-row step."""
    from item_alignment_amd import _lib
    from item_alignment_amd.models import functional as Fn
    lib = _lib.load()
    model, cfg, batch = coca_model
    text = model.coca.text_encoder
    ids, tts = batch[0], batch[2]
    mask = batch[1].clone()
    mask[2, 0] = 0                                   # sequence 2: position 0 masked, later positions attended
    assert mask[2].any()
    lists = Fn.cls_row_lists(mask.shape[0], mask.shape[1], mask.device, (mask != 0).to(torch.uint8))
    live = lists.buf[: mask.numel()].view(mask.shape)
    assert live[:, 1:].sum().item() == 0 and live[2, 0].item() == 0 and live[:, 0].sum().item() == mask.shape[0] - 1

    def step(on):
        was = lib.ia_debug_out_rows(1 if on else 0)
        try:
            model.train()
            Fn.set_step_seed(77)
            model.param_arena.zero_grad()
            hs = text(ids, attention_mask=mask, token_type_ids=tts, padded_rows_unread=True, cls_only_read=True).last_hidden_state
            cls = hs[:, 0].clone()
            hs[:, 0].float().sum().backward()
            grads = {n: p.grad.detach().clone() for n, p in text.named_parameters() if p.grad is not None}
            torch.cuda.synchronize()
        finally:
            lib.ia_debug_out_rows(was)
        return cls, grads
    (c_on, g_on), (c_off, g_off) = step(True), step(False)
    assert torch.isfinite(c_on.float()).all() and torch.equal(c_on, c_off)
    assert c_on[2].float().abs().max().item() == 0.0 and c_on[0].float().abs().max().item() > 0.0
    assert g_on.keys() == g_off.keys() and any(v.abs().max().item() > 0 for v in g_on.values())
    for n in g_on:
        assert torch.isfinite(g_on[n]).all(), n
        assert torch.equal(g_on[n], g_off[n]), n
