"""fp64 restatement (torch, CPU) of the graph model of the reference's src/models/graph.py, with the dropout masks passed in.

torch_geometric is not installable here, so GCN2Conv is restated from its published definition with the reference's arguments
(shared_weights=True, normalize=False, layer l = 1..L):
    beta_l = log(theta / l + 1);  h = (1 - alpha) A x + alpha x_0;  out = (1 - beta_l) h + beta_l (h @ W_l)
and GCN.forward is  dropout(X) -> x = x_0 = relu(linear(X));  x = relu(conv(dropout(x), x_0, A)) per layer;  dropout(x).

Every kernel-level function returns (value, S): S is the same expression evaluated on absolute values, the scale an fp32
evaluation's rounding error is proportional to (|got - ref| <= tau * S with tau = (n + 4) * 2^-24, n the longest sum).

The masks are those of csrc/common.h's counter hash: element e of stream s is kept iff the 16-bit half (e & 1) of
ia_rng(seed, s, e >> 1) is >= thr16 = round(p * 65536); kept elements are scaled by 1 / (1 - thr16 / 65536).
"""
import math

import numpy as np
import torch

F64 = torch.float64
STREAM_INPUT, STREAM_HEAD = 3000, 3100
U = 2.0 ** -24


# ------------------------------------------------------------------------------------------------ the dropout hash on the host
def _mix32(x):
    x = x.astype(np.uint64)
    m = np.uint64(0xFFFFFFFF)
    x ^= x >> np.uint64(16); x = (x * np.uint64(0x7feb352d)) & m
    x ^= x >> np.uint64(15); x = (x * np.uint64(0x846ca68b)) & m
    x ^= x >> np.uint64(16)
    return x


def keep_mask(seed, stream, n, p):
    """(keep [n] float64 of 0 / 1, scale) of a dropout with probability p over elements 0 .. n-1."""
    if p <= 0:
        return torch.ones(n, dtype=F64), 1.0
    thr = int(np.float32(p) * np.float32(65536.0) + np.float32(0.5))
    key = _mix32(np.asarray([(int(stream) ^ ((int(seed) * 0x9E3779B9) & 0xFFFFFFFF)) & 0xFFFFFFFF], dtype=np.uint64))[0]
    idx = np.arange((n + 1) // 2, dtype=np.uint64)
    r = _mix32(idx ^ key)
    u = np.stack([r & np.uint64(0xFFFF), r >> np.uint64(16)], 1).reshape(-1)[:n]
    scale = float(np.float32(1.0) / (np.float32(1.0) - np.float32(thr) / np.float32(65536.0)))
    return torch.from_numpy((u >= thr).astype(np.float64)), scale


def beta_of(theta, layer):
    return math.log(theta / layer + 1)


# ------------------------------------------------------------------------------------------------ kernel-level pieces
def _spmm(A, x):
    return torch.sparse.mm(A, x) if A.is_sparse else A @ x


def _abs(A):
    if A.is_sparse:
        A = A.coalesce()
        return torch.sparse_coo_tensor(A.indices(), A.values().abs(), A.shape).coalesce()
    return A.abs()


def propagate_fwd(A, x, x0, alpha, keep=None, scale=1.0):
    """h = (1 - alpha) A (keep * x * scale) + alpha x0"""
    xd = x if keep is None else x * keep.view_as(x) * scale
    h = (1 - alpha) * _spmm(A, xd) + alpha * x0
    S = (1 - alpha) * _spmm(_abs(A), xd.abs()) + alpha * x0.abs()
    return h, S


def propagate_bwd(A, dh, alpha, keep=None, scale=1.0, dx0_prior=None):
    """dx = keep * scale * (1 - alpha) A^T dh;  dx0 = prior + alpha dh"""
    At = A.t().coalesce() if A.is_sparse else A.t()
    k = 1.0 if keep is None else keep.view_as(dh) * scale
    dx = k * (1 - alpha) * _spmm(At, dh)
    Sx = k * (1 - alpha) * _spmm(_abs(At), dh.abs())
    dx0 = alpha * dh + (0 if dx0_prior is None else dx0_prior)
    S0 = alpha * dh.abs() + (0 if dx0_prior is None else dx0_prior.abs())
    return dx, Sx, dx0, S0


def mix_fwd(h, W, beta, keep=None, scale=1.0):
    """out = keep * scale * relu((1 - beta) h + beta h W)"""
    k = 1.0 if keep is None else keep.view_as(h) * scale
    pre = (1 - beta) * h + beta * (h @ W)
    S = k * ((1 - beta) * h.abs() + beta * (h.abs() @ W.abs()))
    return k * torch.relu(pre), S, pre


def mix_bwd(dout, out, h, W, beta, scale=1.0):
    """dpre = dout * (out > 0) * scale;  dh = (1 - beta) dpre + beta dpre W^T;  dW = beta h^T dpre"""
    dpre = dout * (out > 0).to(F64) * scale
    dh = (1 - beta) * dpre + beta * (dpre @ W.t())
    Sh = (1 - beta) * dpre.abs() + beta * (dpre.abs() @ W.abs().t())
    dW = beta * (h.t() @ dpre)
    SW = beta * (h.abs().t() @ dpre.abs())
    return dh, Sh, dW, SW


def input_fwd(X, W, b, keep=None, scale=1.0):
    Xd = X if keep is None else X * keep.view_as(X) * scale
    pre = Xd @ W.t() + b
    return torch.relu(pre), Xd.abs() @ W.abs().t() + b.abs()


def input_bwd(dx0, x0, X, keep=None, scale=1.0):
    Xd = X if keep is None else X * keep.view_as(X) * scale
    dpre = dx0 * (x0 > 0).to(F64)
    return dpre.t() @ Xd, dpre.abs().t() @ Xd.abs(), dpre.sum(0), dpre.abs().sum(0)


# ------------------------------------------------------------------------------------------------ the whole model
def masks_for(seed, p, N, F, C, L, R):
    """The L + 3 masks of one training step: 'input' [N, F], 'layer' l = 0 .. L-1 [N, C], 'output' [N, C], 'head' [R, C]."""
    m = {"input": keep_mask(seed, STREAM_INPUT, N * F, p)[0].view(N, F), "output": keep_mask(seed, STREAM_INPUT + L + 1, N * C, p)[0].view(N, C),
         "head": keep_mask(seed, STREAM_HEAD, R * C, p)[0].view(R, C), "scale": keep_mask(seed, 0, 2, p)[1]}
    m["layer"] = [keep_mask(seed, STREAM_INPUT + 1 + l, N * C, p)[0].view(N, C) for l in range(L)]
    return m


def gcn_forward(params, X, A, alpha, theta, masks=None):
    """params: dict with the reference's state_dict keys (fp64 tensors).  Returns node embeddings and the stash of the backward."""
    L = sum(1 for k in params if k.startswith("encoder.convs."))
    sc = 1.0 if masks is None else masks["scale"]
    x0, _ = input_fwd(X, params["encoder.linear.weight"], params["encoder.linear.bias"], None if masks is None else masks["input"], sc)
    x, hs, xs = x0, [], []
    for l in range(L):
        h, _ = propagate_fwd(A, x, x0, alpha, None if masks is None else masks["layer"][l], sc)
        last = l == L - 1
        out, _, _ = mix_fwd(h, params[f"encoder.convs.{l}.weight1"], beta_of(theta, l + 1), masks["output"] if (masks is not None and last) else None,
                            sc if last else 1.0)
        hs.append(h); xs.append(out)
        x = out
    return x, dict(x0=x0, hs=hs, xs=xs, X=X, A=A, alpha=alpha, theta=theta, masks=masks, L=L)


def gcn_backward(params, st, dnode):
    L, masks, A, alpha = st["L"], st["masks"], st["A"], st["alpha"]
    sc = 1.0 if masks is None else masks["scale"]
    grads, d, dx0 = {}, dnode, None
    for l in range(L - 1, -1, -1):
        last = l == L - 1
        dh, _, dW, _ = mix_bwd(d, st["xs"][l], st["hs"][l], params[f"encoder.convs.{l}.weight1"], beta_of(st["theta"], l + 1),
                               sc if (masks is not None and last) else 1.0)
        grads[f"encoder.convs.{l}.weight1"] = dW
        dx, _, dx0, _ = propagate_bwd(A, dh, alpha, None if masks is None else masks["layer"][l], sc, dx0)
        d = dx
    dx0 = dx0 + d                                   # layer 1 reads x_0 itself
    dW, _, db, _ = input_bwd(dx0, st["x0"], st["X"], None if masks is None else masks["input"], sc)
    grads["encoder.linear.weight"], grads["encoder.linear.bias"] = dW, db
    return grads


def two_tower(params, X, A, src, tgt, labels, alpha, theta, pairwise, masks=None, want_grads=True):
    """GCNTwoTower.forward and its hand-derived backward.  src / tgt: lists of node indices; labels: list of ints or None.
    pairwise=False is the reference's literal form (quirk G1): every label is scored against the logits of pair 0."""
    node, st = gcn_forward(params, X, A, alpha, theta, masks)
    P = len(src)
    idx = torch.tensor(list(src) + list(tgt), dtype=torch.long)
    k = 1.0 if masks is None else masks["head"] * masks["scale"]
    feats = node[idx] * k
    cat = torch.cat((feats[:P], feats[P:]), 1)
    W, b = params["classifier.out_proj.weight"], params["classifier.out_proj.bias"]
    logits_all = cat @ W.t() + b
    prob = torch.softmax(logits_all, 1)
    out = dict(node=node, logits=logits_all if pairwise else logits_all[:1], probs=prob[:, 1], src_embeds=prob[:, 0], tgt_embeds=prob[:, 1],
               loss=None, grads=None)
    if labels is None:
        return out
    y = torch.tensor(labels, dtype=torch.long)
    onehot = torch.nn.functional.one_hot(y, W.shape[0]).to(F64)
    lg = logits_all if pairwise else logits_all[:1].expand(P, -1)
    logp = torch.log_softmax(lg, 1)
    out["loss"] = -(logp * onehot).sum(1).mean()
    if not want_grads:
        return out
    dlg = (torch.softmax(lg, 1) - onehot) / P                      # d loss / d lg, row k
    if not pairwise:
        dl = torch.zeros_like(logits_all)
        dl[0] = dlg.sum(0)
        dlg = dl
    grads = {"classifier.out_proj.weight": dlg.t() @ cat, "classifier.out_proj.bias": dlg.sum(0)}
    dcat = dlg @ W
    dfe = torch.cat((dcat[:, :W.shape[1] // 2], dcat[:, W.shape[1] // 2:]), 0) * k
    dnode = torch.zeros_like(node)
    dnode.index_add_(0, idx, dfe)
    grads.update(gcn_backward(params, st, dnode))
    out["grads"] = grads
    return out


def adamw_steps(params, grads_fn, steps, lr, total, warm, betas=(0.9, 0.98), eps=1e-8, wd=1e-5):
    """torch.optim.AdamW with the reference's two parameter groups (no decay on names holding 'bias') under
    get_linear_schedule_with_warmup, in fp64.  grads_fn(params) -> dict of gradients."""
    m = {k: torch.zeros_like(v) for k, v in params.items()}
    v = {k: torch.zeros_like(p) for k, p in params.items()}
    params = {k: p.clone() for k, p in params.items()}
    for t in range(1, steps + 1):
        s = t - 1
        mult = s / max(1, warm) if s < warm else max(0.0, (total - s) / max(1, total - warm))
        g = grads_fn(params)
        for k in params:
            decay = 0.0 if "bias" in k else wd
            params[k] = params[k] * (1 - lr * mult * decay)
            m[k] = betas[0] * m[k] + (1 - betas[0]) * g[k]
            v[k] = betas[1] * v[k] + (1 - betas[1]) * g[k] * g[k]
            mh, vh = m[k] / (1 - betas[0] ** t), v[k] / (1 - betas[1] ** t)
            params[k] = params[k] - lr * mult * mh / (vh.sqrt() + eps)
    return params
