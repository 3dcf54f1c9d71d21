"""tests/textcnn_reference.py (the fp64 restatement the GPU kernel tests compare against) checked on the host: against autograd of
F.conv2d -> relu -> max_pool1d in fp64, and against the reference project's own gradient in tests/golden/textcnn_two_tower.npz."""
import pytest
import torch
import torch.nn.functional as F

import textcnn_reference as T
from golden_util import load_case, weights

F64 = torch.float64
SHAPES = [(1, 5, 8, 1, "5"), (3, 6, 16, 4, "1,2,3,5"), (2, 20, 24, 6, "1,2,3,5"), (2, 17, 8, 5, "3")]


def _inputs(B, L, H, nF, sizes, seed):
    g = torch.Generator().manual_seed(seed)
    x0, x1 = (torch.randn((B * L, H), generator=g, dtype=F64) for _ in range(2))
    Ws = [torch.randn((nF, 2, K, H), generator=g, dtype=F64) / (2 * K * H) ** 0.5 for K in sizes]
    bs = [torch.randn(nF, generator=g, dtype=F64) * 0.1 for _ in sizes]
    gr = torch.randn((B, nF * len(sizes)), generator=g, dtype=F64)
    return x0, x1, Ws, bs, gr


def _torch_features(x0, x1, Ws, bs, B, L):
    x = torch.stack((x0.reshape(B, L, -1), x1.reshape(B, L, -1)), dim=1)
    outs = [F.relu(F.conv2d(x, w, b)).squeeze(3) for w, b in zip(Ws, bs)]
    return torch.cat([F.max_pool1d(o, o.size(2)).squeeze(2) for o in outs], 1)


@pytest.mark.parametrize("B,L,H,nF,sizes", SHAPES)
def test_reference_matches_autograd_in_fp64(B, L, H, nF, sizes):
    sizes = T.parse_sizes(sizes)
    x0, x1, Ws, bs, gr = _inputs(B, L, H, nF, sizes, 11)
    for t in [x0, x1] + Ws + bs:
        t.requires_grad_(True)
    feat_t = _torch_features(x0, x1, Ws, bs, B, L)
    (feat_t * gr).sum().backward()
    with torch.no_grad():
        P = T.project(x0, x1, T.pack_taps(Ws, sizes))
        feat, arg, _smax, _gap = T.pool_fwd(P, bs, sizes, B, L)
        assert torch.allclose(feat, feat_t, rtol=1e-9, atol=1e-12)
        assert ((arg >= 0) == (feat_t > 0)).all()
        dW, db, _mw, _mb = T.pool_bwd_w(gr, arg, x0, x1, sizes, L)
        dx, _m = T.pool_bwd_x(gr, arg, Ws, sizes, L)
        for s in range(len(sizes)):
            assert torch.allclose(dW[s], Ws[s].grad, rtol=1e-9, atol=1e-12), s
            assert torch.allclose(db[s], bs[s].grad, rtol=1e-9, atol=1e-12), s
        assert torch.allclose(dx, x0.grad, rtol=1e-9, atol=1e-12)


def test_ties_go_to_the_lowest_t_like_max_pool1d():
    """every input row the same: all windows of a feature tie, the reference (and F.max_pool1d on the CPU) picks t = 0"""
    B, L, H, nF, sizes = 2, 9, 8, 3, [1, 2, 3]
    _x0, _x1, Ws, bs, _g = _inputs(B, L, H, nF, sizes, 5)
    row = torch.randn((1, H), generator=torch.Generator().manual_seed(2), dtype=F64)
    x0 = x1 = row.expand(B * L, H).contiguous()
    bs = [b.abs() + 10.0 for b in bs]                        # every feature alive
    P = T.project(x0, x1, T.pack_taps(Ws, sizes))
    _feat, arg, _s, _gap = T.pool_fwd(P, bs, sizes, B, L)
    x = torch.stack((x0.reshape(B, L, H), x1.reshape(B, L, H)), dim=1)
    for s, (w, b) in enumerate(zip(Ws, bs)):
        o = F.relu(F.conv2d(x, w, b)).squeeze(3)
        _v, idx = F.max_pool1d(o, o.size(2), return_indices=True)
        assert (idx.squeeze(2) == 0).all() and (arg[:, s * nF:(s + 1) * nF] == 0).all()


def test_dead_feature_sends_no_gradient():
    B, L, H, nF, sizes = 2, 7, 8, 2, [2, 3]
    x0, x1, Ws, bs, gr = _inputs(B, L, H, nF, sizes, 3)
    bs[1][0] = -1e4
    P = T.project(x0, x1, T.pack_taps(Ws, sizes))
    feat, arg, _s, _g = T.pool_fwd(P, bs, sizes, B, L)
    j = 1 * nF + 0
    assert (feat[:, j] == 0).all() and (arg[:, j] == -1).all()
    dW, db, _mw, _mb = T.pool_bwd_w(gr, arg, x0, x1, sizes, L)
    assert (dW[1][0] == 0).all() and db[1][0] == 0


def test_reference_reproduces_the_golden_conv_gradient():
    """grad_textcnn.convs1.2.weight of the reference project's TextCNNTwoTower (tests/golden/textcnn_two_tower.npz) out of the hand-derived
    backward: embeddings from the product class on the CPU, tower and head in fp64"""
    import item_alignment_amd.models as M
    from test_models_gpu import cfg_of
    case = load_case("textcnn_two_tower")
    model = M.TextCNNTwoTower(cfg_of(case), {})
    model.load_state_dict(weights(case), strict=False)
    model.eval()
    tc, i = model.textcnn, case.inputs
    sizes = T.parse_sizes(case.cfg.filter_sizes)
    Ws, bs = [c.weight.detach().to(F64) for c in tc.convs1], [c.bias.detach().to(F64) for c in tc.convs1]
    taps = T.pack_taps(Ws, sizes)
    towers = []
    with torch.no_grad():
        for ids in (i["input_ids_1"], i["input_ids_2"]):
            B, L = ids.shape
            x0, x1 = (e(ids).reshape(B * L, -1).to(F64) for e in (tc.embedding1, tc.embedding2))
            feat, arg, _s, _g = T.pool_fwd(T.project(x0, x1, taps), bs, sizes, B, L)
            towers.append((x0, x1, feat.requires_grad_(True), arg, L))
    head = model.classifier.out_proj
    logits = F.linear(torch.cat((towers[0][2], towers[1][2]), 1), head.weight.detach().to(F64), head.bias.detach().to(F64))
    loss = F.cross_entropy(logits, i["labels"])
    assert abs(float(loss.detach()) - float(case.outs["loss"])) < 1e-5
    loss.backward()
    total = sum(T.pool_bwd_w(f.grad, arg, x0, x1, sizes, L)[0][2] for x0, x1, f, arg, L in towers)
    want = case.grads["textcnn.convs1.2.weight"].to(F64)
    assert torch.allclose(total, want, atol=1e-5, rtol=1e-4), float((total - want).abs().max())


@pytest.mark.parametrize("shape", T.KERNEL_SHAPES, ids=T.shape_id)
def test_seeded_kernel_inputs_leave_few_routing_decisions_near_a_tie(shape):
    """tests/test_textcnn_kernels_gpu.py excuses the argmax of a feature whose fp64 gap to the runner-up (or to 0) is inside the fp32
    error bound of the forward kernel; at most 2 % of the entries may be excused, and the seeded inputs alone must stay under that."""
    c = T.seeded_case(shape)
    _feat, arg, smax, gap = T.pool_fwd(c.P, c.bs, c.sizes, c.B, c.L)
    excused = gap <= T.fwd_bound(c.sizes, c.F, smax)
    assert float(excused.to(F64).mean()) <= 0.02, int(excused.sum())
    assert (arg >= 0).any()
