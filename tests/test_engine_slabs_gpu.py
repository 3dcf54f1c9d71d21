"""Two post-LN layers under ia_layer_cfg::masked_rows_dead = 3 with the row filter in 8-row slabs (the forward's four GEMMs and the three
plain data gradients of ia_layer_bwd2) against the same calls with every row computed (ia_debug_fwd_rows(0) / ia_debug_dgrad_rows(0)):
y, every stash buffer at the live rows, dx, dx2 and every parameter gradient bit for bit, and everything finite everywhere with the stash,
the scratch and the outputs filled with 0xFF (NaN as bf16 and as fp32) first.

Two layers: the second reads the first one's y, zeros at the masked positions included, and hands its dx / dx2 down as the first one's
dy / dy2.  Ragged right-padded masks with one sequence of full length and one of length 1.  Dropout on, fixed seed.

Shapes.  B = 3, L in {41, 255}, H = 128, nh = 2, I = 512: the layer calls, the list builders and the new bit at the smallest size; its
GEMMs stay below the 160 tiles from which the 256-wide kernels -- the ones that filter -- serve a call (asserted), so it pins the
contract on the path that computes every row.  B = 40, L = 255, H = 1024, nh = 16, I = 1024 (tests/test_engine_fwd_rows_gpu.py) is the
smallest layer whose GEMMs all filter (asserted): there the slab kernels run.  M = 10200 is no multiple of 128, so the QKV projection's
scaled columns take the guarded one-tile launch on the last rows; 10200 = 8 x 1275: the last slab is whole, the sequences' ends are not.

Each case runs once with the engine building its lists and once with the lists handed in: ia_row_blocks and ia_row_slabs of the mask in
ia_layer_cfg::key_rows.blocks / .slabs."""
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu


def al(b):
    return (b + 255) // 256 * 256


def stash_views(stash, B, L, H, I, NH):
    """the buffers of carve_stash (engine.hip) by name, in carve order"""
    M = B * L
    sizes = [("qkv", M * 3 * H * 2, torch.bfloat16, (M, 3 * H)), ("ctx", M * H * 2, torch.bfloat16, (M, H)), ("z1", M * H * 2, torch.bfloat16, (M, H)),
             ("y1", M * H * 2, torch.bfloat16, (M, H)), ("z2", M * H * 2, torch.bfloat16, (M, H)), ("hpre", M * I * 2, torch.bfloat16, (M, I)),
             ("hact", M * I * 2, torch.bfloat16, (M, I)), ("lse", B * NH * L * 4, torch.float32, (B, NH, L)), ("mean1", M * 4, torch.float32, (M,)),
             ("rstd1", M * 4, torch.float32, (M,)), ("mean2", M * 4, torch.float32, (M,)), ("rstd2", M * 4, torch.float32, (M,))]
    out, off = {}, 0
    for name, nbytes, dt, shape in sizes:
        out[name] = stash[off: off + nbytes].view(dt).view(shape)
        off += al(nbytes)
    return out


CASES = [(3, 41, 128, 2, 512, False), (3, 255, 128, 2, 512, False), (40, 255, 1024, 16, 1024, True)]


@pytest.mark.parametrize("handed_in", [False, True], ids=["engine_lists", "caller_lists"])
@pytest.mark.parametrize("B,L,H,NH,I,filters", CASES)
def test_two_layers_slab_path_equals_dense(gpu, B, L, H, NH, I, filters, handed_in):
    from item_alignment_amd import _lib
    from item_alignment_amd._lib import LayerCfg, LayerGrads, LayerWeights
    from test_engine_gpu import make_layer
    lib = _lib.load()
    M = B * L
    want = [1, 1, 1, 1] if filters else [0, 0, 0, 0]
    assert [lib.ia_gemm_fwd_rows_filters(M, n, k) for n, k in ((3 * H, H), (H, H), (I, H), (H, I))] == want
    assert [lib.ia_gemm_dgrad_rows_filters(M, n, k) for n, k in ((H, I), (H, H), (H, 3 * H))] == want[:3]
    mats = ("w_qkv", "w_o", "w_fc1", "w_fc2")
    layers = []
    for i in range(2):
        P32 = make_layer(H, I, gpu, 3 + i)
        Pb = {k: v.to(torch.bfloat16) for k, v in P32.items() if k in mats}
        Pt = {k: v.t().contiguous() for k, v in Pb.items()}
        w = LayerWeights()
        for k in P32:
            setattr(w, k, (Pb[k] if k in mats else P32[k]).data_ptr())
        for k in mats:
            setattr(w, "wt_" + k[2:], Pt[k].data_ptr())
        layers.append((P32, Pb, Pt, w))
    x = torch.randn(B, L, H, generator=torch.Generator().manual_seed(5)).to(gpu).to(torch.bfloat16)
    ragged = [L, 1, 27, 130, 200, 9, 101, 33, 180, 64]                       # one sequence of full length, one of length 1
    lens = torch.tensor([min(L, ragged[i % len(ragged)]) for i in range(B)])
    mask = (torch.arange(L)[None] < lens[:, None]).to(torch.uint8).to(gpu)
    valid = mask.bool().view(-1)
    dy = torch.randn(M, H, generator=torch.Generator().manual_seed(6)).to(gpu).to(torch.bfloat16)
    dy = (dy * valid[:, None].to(dy.dtype)).contiguous()          # zero at masked positions: what masked_rows_dead promises
    st = torch.cuda.current_stream().cuda_stream
    cfgs = [LayerCfg(B=B, L=L, H=H, I=I, nh=NH, pre_ln=0, eps=1e-12, hidden_drop=0.1, attn_drop=0.1, seed=11, layer_id=i, masked_rows_dead=3)
            for i in range(2)]
    lists = None
    if handed_in:
        lists = [torch.full((getattr(lib, f"ia_{name}_bytes")(M),), 0xFF, device=gpu, dtype=torch.uint8) for name in ("row_blocks", "row_slabs")]
        _lib.check(lib.ia_row_blocks(mask.data_ptr(), M, lists[0].data_ptr(), st), "ia_row_blocks")
        _lib.check(lib.ia_row_slabs(mask.data_ptr(), M, lists[1].data_ptr(), st), "ia_row_slabs")
        for c in cfgs:
            c.key_rows.blocks, c.key_rows.slabs = lists[0].data_ptr(), lists[1].data_ptr()

    def run(skip):
        was_f, was_d = lib.ia_debug_fwd_rows(1 if skip else 0), lib.ia_debug_dgrad_rows(1 if skip else 0)
        try:
            cur, ys, stashes = x, [], []
            for i in range(2):
                stash = torch.full((lib.ia_layer_stash_bytes(C.byref(cfgs[i])),), 0xFF, device=gpu, dtype=torch.uint8)
                y = torch.full((M, H), -1, device=gpu, dtype=torch.int16).view(torch.bfloat16)
                _lib.check(lib.ia_layer_fwd(C.byref(cfgs[i]), C.byref(layers[i][3]), cur.data_ptr(), mask.data_ptr(), y.data_ptr(), stash.data_ptr(), st),
                           f"fwd[{i}] (skip={skip})")
                ys.append(y); stashes.append(stash)
                cur = y
            grads, g_in, g_in2 = [None, None], dy, None
            dxs = []
            for i in (1, 0):
                scratch = torch.full((lib.ia_layer_bwd_scratch_bytes(C.byref(cfgs[i])),), 0xFF, device=gpu, dtype=torch.uint8)
                G = {k: torch.zeros_like(v) for k, v in layers[i][0].items()}
                g = LayerGrads()
                for k in G:
                    setattr(g, k, G[k].data_ptr())
                dx = torch.full_like(dy, float("nan"))
                dx2 = torch.full_like(dy, float("nan"))
                xin = x if i == 0 else ys[0]
                _lib.check(lib.ia_layer_bwd2(C.byref(cfgs[i]), C.byref(layers[i][3]), C.byref(g), xin.data_ptr(), mask.data_ptr(), ys[i].data_ptr(),
                                             stashes[i].data_ptr(), g_in.data_ptr(), g_in2.data_ptr() if g_in2 is not None else None, dx.data_ptr(),
                                             dx2.data_ptr(), scratch.data_ptr(), scratch.numel(), st), f"bwd2[{i}] (skip={skip})")
                grads[i] = G
                dxs.append((dx, dx2))
                g_in, g_in2 = dx, dx2
            torch.cuda.synchronize()
        finally:
            lib.ia_debug_fwd_rows(was_f); lib.ia_debug_dgrad_rows(was_d)
        return ys, stashes, dxs, grads

    ys_d, st_d, dx_d, g_d = run(False)
    ys_s, st_s, dx_s, g_s = run(True)
    for i in range(2):
        assert torch.isfinite(ys_s[i].float()).all(), ("y", i)
        assert torch.equal(ys_d[i][valid], ys_s[i][valid]), ("y", i)
        assert ys_s[i][~valid].float().abs().max().item() == 0.0, ("y", i)      # masked positions leave as zeros
        vd, vs = stash_views(st_d[i], B, L, H, I, NH), stash_views(st_s[i], B, L, H, I, NH)
        for name in vd:
            a, b = vd[name], vs[name]
            assert torch.isfinite(b.float()).all(), (name, i)                 # the backward reads every row of some of them
            if name == "lse":
                live = mask.bool()[:, None, :].expand(B, NH, L)
                assert torch.equal(a[live], b[live]), (name, i)
            else:
                assert torch.equal(a[valid], b[valid]), (name, i)
    for j, i in enumerate((1, 0)):
        for name, a, b in (("dx", dx_d[j][0], dx_s[j][0]), ("dx2", dx_d[j][1], dx_s[j][1])):
            assert torch.isfinite(b.float()).all(), (name, i)
            assert torch.equal(a, b), (name, i)
        assert dx_s[j][0][~valid].float().abs().max().item() == 0.0, ("dx", i)     # dead rows leave as zeros
        for k in g_d[i]:
            assert g_d[i][k].abs().max().item() > 0.0, (k, i)
            assert torch.equal(g_d[i][k], g_s[i][k]), (k, i)
    del lists
