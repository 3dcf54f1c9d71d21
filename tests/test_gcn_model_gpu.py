"""GCNTwoTower on the GPU against the fp64 restatement (tests/gcn_reference.py) and the golden file written from the
reference's own wrapper by tools/gen_golden_gcn.py (tests/golden/gcn/).

Bound: the model is a chain of sums -- F terms in the input layer, then per layer a row sum of at most d_max neighbours and a C-term
product, then 2 C terms in the head -- so an output carries at most n = F + L (d_max + C) + 2 C + 4 (L + 2) fp32 roundings relative
to the scale of its tensor; tau = n * 2^-24 against max |ref| of the tensor (gradients: twice the chain, forward and backward).  This
bound is tensor-relative, not per element: through relu and softmax there is no "same expression on absolute values", so a small
element is held to the tensor's scale here; the per-element form is what tests/test_gcn_kernels_gpu.py applies to every kernel.  The
optimiser trajectory uses the tolerance of tests/test_optim_gpu.py (the sign-like first Adam steps amplify relative gradient error).
"""
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import gcn_reference as R

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "gcn", "gcn_two_tower.npz")
U = 2.0 ** -24
KEYS = ["encoder.linear.weight", "encoder.linear.bias", "classifier.out_proj.weight", "classifier.out_proj.bias"]


def fixture():
    """The committed golden problem (tools/gen_golden_gcn.py): a missing file is an error, never a reason to test something else."""
    g = np.load(GOLD)
    N, F, C, L = int(g["N"]), int(g["F"]), int(g["C"]), int(g["L"])
    X, ei = torch.from_numpy(g["X"]), torch.from_numpy(g["edge_index"])
    src, tgt, labels = g["src"].tolist(), g["tgt"].tolist(), g["labels"].tolist()
    params = {k[2:]: torch.from_numpy(g[k]) for k in g.files if k.startswith("w.")}
    cfg = SimpleNamespace(hidden_size=F, intermediate_size=C, num_hidden_layers=L, hidden_dropout_prob=0.1, num_labels=2, alpha=0.1, theta=0.5,
                          loss_type="ce", num_entities=N)
    pairs = [{"src_idx": s, "tgt_idx": t, "src_item_id": f"a{s}", "tgt_item_id": f"b{t}", "item_label": str(y)} for s, t, y in zip(src, tgt, labels)]
    return cfg, params, X, ei, pairs


def make_model(cfg, params, pairwise, monkeypatch):
    import item_alignment_amd.models as M
    monkeypatch.setenv("IA_GCN_PAIRWISE_LOSS", "1" if pairwise else "0")
    model = M.GCNTwoTower(cfg)
    assert sorted(model.state_dict()) == sorted(params)
    model.load_state_dict(params)
    return model.cuda()


def dense_ref(cfg, params, X, ei, pairs, pairwise, masks=None):
    N = X.shape[0]
    A = torch.sparse_coo_tensor(torch.stack((ei[1], ei[0])), torch.ones(ei.shape[1], dtype=R.F64), (N, N)).coalesce()
    p64 = {k: v.double() for k, v in params.items()}
    return R.two_tower(p64, X.double(), A, [p["src_idx"] for p in pairs], [p["tgt_idx"] for p in pairs], [int(p["item_label"]) for p in pairs],
                       cfg.alpha, cfg.theta, pairwise, masks), A


def chain_tau(cfg, A, grad=False):
    dmax = float(torch.bincount(A.indices()[0]).max())
    n = cfg.hidden_size + cfg.num_hidden_layers * (dmax + cfg.intermediate_size) + 2 * cfg.intermediate_size + 4 * (cfg.num_hidden_layers + 2)
    return (2 if grad else 1) * n * U


def close(name, got, ref, tau):
    got, ref = got.detach().double().cpu().reshape(-1), ref.double().reshape(-1)
    scale = float(ref.abs().max())
    err = float((got - ref).abs().max())
    print(f"GCN-BOUND model {name:28s} max|err|/max|ref| = {err / max(scale, 1e-300) / U:10.2f} * 2^-24   (bound {tau / U:.0f})")
    assert err <= tau * scale + 1e-300, (name, err, tau * scale)


@pytest.mark.parametrize("pairwise", [False, True])
def test_forward_backward_and_three_steps(pairwise, monkeypatch):
    from item_alignment_amd.models import load_adjacency
    from item_alignment_amd.train import ArenaAdamW, linear_schedule_with_warmup
    cfg, params, X, ei, pairs = fixture()
    assert len({p["src_idx"] for p in pairs} & {p["tgt_idx"] for p in pairs}) >= 2          # nodes shared between pairs
    model = make_model(cfg, params, pairwise, monkeypatch).eval()
    adj = load_adjacency(ei, num_nodes=X.shape[0], device="cuda")
    Xg = X.cuda()
    ref, A = dense_ref(cfg, params, X, ei, pairs, pairwise)
    tau, taug = chain_tau(cfg, A), chain_tau(cfg, A, grad=True)
    out = model(Xg, adj, pairs)
    node = model.encoder(Xg, adj)
    close("node_embeddings", node, ref["node"], tau)
    assert out.logits.shape == ((len(pairs), 2) if pairwise else (1, 2))
    for k in ("logits", "probs", "src_embeds", "tgt_embeds", "loss"):
        close(k, out[k], ref[k], tau)
    model.param_arena.zero_grad()
    out.loss.backward()
    got = {k: v.grad.clone() for k, v in model.named_parameters()}
    for k, g in got.items():
        close("grad " + k, g, ref["grads"][k], taug)
    # eval mode is reproducible bit for bit, gradients included
    model.param_arena.zero_grad()
    out2 = model(Xg, adj, pairs)
    out2.loss.backward()
    assert torch.equal(out2.probs, out.probs) and torch.equal(out2.loss, out.loss)
    for k, v in model.named_parameters():
        assert torch.equal(v.grad, got[k]), k
    # three AdamW + schedule steps (lr 1e-3, betas (0.9, 0.98), wd 1e-5, warm-up 1 of 10 steps)
    model.param_arena.zero_grad()
    opt = ArenaAdamW(model, 1e-3, 1e-8, 1e-5)
    for s in range(3):
        model(Xg, adj, pairs).loss.backward()
        opt.step(linear_schedule_with_warmup(s, 1, 10))
        opt.zero_grad()
    p64 = {k: v.double() for k, v in params.items()}
    srcs, tgts, ys = [p["src_idx"] for p in pairs], [p["tgt_idx"] for p in pairs], [int(p["item_label"]) for p in pairs]
    want = R.adamw_steps(p64, lambda q: R.two_tower(q, X.double(), A, srcs, tgts, ys, cfg.alpha, cfg.theta, pairwise)["grads"], 3, 1e-3, 10, 1)
    for k, v in model.named_parameters():
        # tests/test_optim_gpu.py tolerance for an AdamW trajectory: 2e-5 absolute + 2e-5 relative per step
        d = (v.detach().double().cpu() - want[k]).abs()
        lim = 3 * (2e-5 + 2e-5 * want[k].abs())
        print(f"GCN-BOUND model steps {k:28s} max |dw| = {float(d.max()):.3e}")
        assert bool((d <= lim).all()), (k, float(d.max()))
    if not pairwise:        # the reference's own fp32 trajectory exists for its literal loss form only
        g = np.load(GOLD)
        for k, v in model.named_parameters():
            w = torch.from_numpy(g["after3.literal." + k]).double()
            d = (v.detach().double().cpu() - w).abs()
            assert bool((d <= 3 * (2e-5 + 2e-5 * w.abs())).all()), (k, float(d.max()))


def test_golden_outputs(monkeypatch):
    from item_alignment_amd.models import load_adjacency
    g = np.load(GOLD)
    cfg, params, X, ei, pairs = fixture()
    model = make_model(cfg, params, False, monkeypatch).eval()
    adj = load_adjacency(ei, num_nodes=X.shape[0], device="cuda")
    _, A = dense_ref(cfg, params, X, ei, pairs, False)
    tau, taug = chain_tau(cfg, A) + 2 * U, chain_tau(cfg, A, grad=True) + 2 * U       # the golden values are themselves fp32
    out = model(X.cuda(), adj, pairs)
    close("golden node", model.encoder(X.cuda(), adj), torch.from_numpy(g["node"]), tau)
    for k in ("logits", "probs", "src_embeds", "tgt_embeds", "loss"):
        close("golden " + k, out[k], torch.from_numpy(g["literal." + k]), tau)
    model.param_arena.zero_grad()
    out.loss.backward()
    for k, v in model.named_parameters():
        close("golden grad " + k, v.grad, torch.from_numpy(g["literal.grad." + k]), taug)


def test_training_mode_dropout(monkeypatch):
    from item_alignment_amd.models import load_adjacency, functional as Fn, graph as G
    cfg, params, X, ei, pairs = fixture()
    model = make_model(cfg, params, True, monkeypatch).train()
    adj = load_adjacency(ei, num_nodes=X.shape[0], device="cuda")
    Xg = X.cuda()
    N, F, C, L = X.shape[0], cfg.hidden_size, cfg.intermediate_size, cfg.num_hidden_layers

    def run(seed):
        Fn.set_step_seed(seed)
        model.param_arena.zero_grad()
        out = model(Xg, adj, pairs)
        out.loss.backward()
        return out.loss.clone(), out.probs.clone(), model.encoder.linear.weight.grad.clone()

    a, b, c = run(11), run(11), run(12)
    assert torch.isfinite(a[0])
    assert all(torch.equal(x, y) for x, y in zip(a, b))
    assert not torch.equal(a[1], c[1])
    # the training step equals the fp64 restatement under the same masks (recomputed on the host from the counter hash)
    masks = R.masks_for(11, cfg.hidden_dropout_prob, N, F, C, L, 2 * len(pairs))
    ref, A = dense_ref(cfg, params, X, ei, pairs, True, masks)
    close("train loss", a[0], ref["loss"], chain_tau(cfg, A))
    close("train grad linear.weight", a[2], ref["grads"]["encoder.linear.weight"], chain_tau(cfg, A, grad=True))
    # keep rate of each of the L + 2 encoder masks, seen through the kernels themselves, within 4 sigma of 1 - p
    from item_alignment_amd import _lib
    lib = _lib.load()
    p, seed = cfg.hidden_dropout_prob, 11
    Nn, Cc = 4096, 128
    ones = torch.ones((Nn, Cc), device="cuda")
    zeros = torch.zeros((Nn, Cc), device="cuda")
    eye = G.load_adjacency(torch.arange(Nn).repeat(2, 1), num_nodes=Nn, device="cuda")
    rates = []
    Wi = torch.eye(Cc, device="cuda")
    o = torch.empty((Nn, Cc), device="cuda")
    assert lib.ia_gcn_input_fwd(ones.data_ptr(), Wi.data_ptr(), zeros.data_ptr(), o.data_ptr(), Nn, Cc, Cc, p, seed, G.STREAM_INPUT, _lib.stream_ptr()) == 0
    rates.append(float((o > 0).float().mean()))
    for l in range(L):
        assert lib.ia_gcn_propagate_fwd(eye.rowptr.data_ptr(), eye.col.data_ptr(), 0, None, ones.data_ptr(), zeros.data_ptr(), o.data_ptr(), Nn, Cc, 0.0,
                                        p, seed, G.STREAM_INPUT + 1 + l, None, 0, _lib.stream_ptr()) == 0
        rates.append(float((o > 0).float().mean()))
    assert lib.ia_gcn_mix_fwd(ones.data_ptr(), zeros.data_ptr(), o.data_ptr(), Nn, Cc, 0.0, p, seed, G.STREAM_INPUT + L + 1, _lib.stream_ptr()) == 0
    rates.append(float((o > 0).float().mean()))
    sigma = (p * (1 - p) / (Nn * Cc)) ** 0.5
    print("GCN-BOUND keep rates", rates, "4 sigma =", 4 * sigma)
    assert len(rates) == L + 2
    for r in rates:
        assert abs(r - (1 - p)) <= 4 * sigma + 1.0 / 65536, rates       # 1 / 65536: the 16-bit threshold's own granularity
    assert len({round(r, 9) for r in rates}) == L + 2                      # different streams, different masks


def test_state_dict_round_trip(monkeypatch, tmp_path):
    cfg, params, X, ei, pairs = fixture()
    model = make_model(cfg, params, False, monkeypatch)
    f = tmp_path / "graph_epoch-0.bin"
    torch.save(model.state_dict(), f)
    sd = torch.load(f, map_location="cpu")
    want = ["classifier.out_proj.bias", "classifier.out_proj.weight", "encoder.linear.bias", "encoder.linear.weight"] + \
           [f"encoder.convs.{i}.weight1" for i in range(cfg.num_hidden_layers)]
    assert sorted(sd) == sorted(want)
    for k in want:
        assert torch.equal(sd[k], params[k])
    model2 = make_model(cfg, {k: torch.zeros_like(v) for k, v in params.items()}, False, monkeypatch)
    model2.load_state_dict(sd)
    for k, v in model2.state_dict().items():
        assert torch.equal(v.cpu(), params[k])


def test_cpu_inputs_raise(monkeypatch):
    from item_alignment_amd._lib import ItemAlignError
    from item_alignment_amd.models import load_adjacency
    cfg, params, X, ei, pairs = fixture()
    model = make_model(cfg, params, False, monkeypatch)
    with pytest.raises(ItemAlignError):
        model(X, load_adjacency(ei, num_nodes=X.shape[0], device="cuda"), pairs)
    with pytest.raises(ItemAlignError):
        model(X.cuda(), load_adjacency(ei, num_nodes=X.shape[0]), pairs)
