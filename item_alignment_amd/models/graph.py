"""Host-side mirror of the reference's src/models/graph.py: GCN (a GCNII encoder over the item / attribute-value graph) and
GCNTwoTower (TwoTowerClassificationHead on the node embeddings of a pair) -- same class names, constructor arguments, forward
signatures and state_dict keys, with the full-graph forward and backward done by the kernels of csrc/gcn.hip.

torch_geometric's GCN2Conv is restated from its published definition (shared_weights=True, normalize=False, layer l = 1..L):
    beta_l = log(theta / l + 1);  h = (1 - alpha) * A @ x + alpha * x_0;  out = (1 - beta_l) * h + beta_l * (h @ weight1)
`A` is adj_t as given: no self loops added, no degree normalisation.

Reference quirks kept:
  G1  graph.py:95-103 stores only the first pair's logits, so the "ce" loss is mean_k CE(logits of pair 0, label_k), `logits` is
      [1, 2] and only pair 0 sends a gradient into the graph.  IA_GCN_PAIRWISE_LOSS=1 (read when the model is built) switches to
      logits [P, 2] and loss = mean_k CE(logits_k, label_k).
  G2  only loss_type "ce" is reachable without an error in the reference; the others raise ValueError here, at construction.
"""
import math
import os

import torch
from torch import nn

from .. import _lib
from .._lib import check, ptr, stream_ptr
from .base import HipModule, SequenceClassifierOutput, TwoTowerClassificationHead
from . import functional as Fn

F32 = torch.float32
LONG_ROW = 512                      # IA_GCN_LONG_ROW of include/itemalign.h
STREAM_INPUT, STREAM_HEAD = 3000, 3100      # dropout streams: input 3000, layer l (1-based) 3000 + l, output 3000 + L + 1, head 3100


# ------------------------------------------------------------------------------------------------ adjacency
class GraphAdjacency:
    """CSR of A and of A^T (rowptr int64 [N+1], col int32 [nnz], val fp32 [nnz] or None = all ones) plus the lists of rows with
    more than LONG_ROW neighbours, on one device.  Built once by load_adjacency; the model only reads it."""

    def __init__(self, n, rowptr, col, val, rowptr_t, col_t, val_t):
        self.num_nodes = int(n)
        self.rowptr, self.col, self.val = rowptr, col, val
        self.rowptr_t, self.col_t, self.val_t = rowptr_t, col_t, val_t
        self.long_rows = _long_rows(rowptr)
        self.long_rows_t = _long_rows(rowptr_t)

    @property
    def nnz(self):
        return int(self.col.numel())

    @property
    def device(self):
        return self.rowptr.device

    @property
    def is_cuda(self):
        return self.rowptr.is_cuda

    def to(self, device):
        mv = lambda t: None if t is None else t.to(device)
        out = object.__new__(GraphAdjacency)
        out.num_nodes = self.num_nodes
        for k in ("rowptr", "col", "val", "rowptr_t", "col_t", "val_t", "long_rows", "long_rows_t"):
            setattr(out, k, mv(getattr(self, k)))
        return out

    def cuda(self):
        return self.to("cuda")


def _long_rows(rowptr):
    deg = rowptr[1:] - rowptr[:-1]
    return torch.nonzero(deg > LONG_ROW).view(-1).to(torch.int32).contiguous()


def _csr_from_coo(row, col, val, n):
    """(row, col, val) with duplicates -> sorted, duplicate-free CSR; duplicate edges are summed."""
    if row.numel() and (int(row.min()) < 0 or int(row.max()) >= n or int(col.min()) < 0 or int(col.max()) >= n):
        raise ValueError(f"adjacency index outside [0, {n})")
    if n >= 2 ** 31:
        raise ValueError("more than 2^31 - 1 nodes")
    v = torch.ones(row.numel(), dtype=F32) if val is None else val.to(F32)
    m = torch.sparse_coo_tensor(torch.stack((row.long(), col.long())), v, (n, n)).coalesce()
    r, c = m.indices()
    v = m.values()
    rowptr = torch.zeros(n + 1, dtype=torch.int64)
    rowptr[1:] = torch.cumsum(torch.bincount(r, minlength=n), 0)
    ones = bool((v == 1).all())
    return rowptr, c.to(torch.int32).contiguous(), (None if ones else v.contiguous())


def load_adjacency(obj, num_nodes=None, device=None):
    """GraphAdjacency from: a GraphAdjacency (returned as it is, moved if `device` says so); a torch sparse COO or CSR tensor
    (square); an integer `edge_index` [2, E], or a tuple (edge_index, values) -- PyG convention: edge (j = edge_index[0, e]) ->
    (i = edge_index[1, e]) puts values[e] at A[i, j]; a (rowptr, col, values-or-None) CSR triple; or a torch_sparse.SparseTensor
    when that package is importable.  Duplicate edges are summed.  `device` defaults to the device the object lives on."""
    if isinstance(obj, GraphAdjacency):
        return obj if device is None else obj.to(device)
    val = None
    if isinstance(obj, (tuple, list)) and len(obj) == 3 and torch.is_tensor(obj[0]) and obj[0].dim() == 1:
        rowptr, col, val = obj
        dev = rowptr.device
        rowptr, col = rowptr.cpu().long(), col.cpu().long()
        n = rowptr.numel() - 1
        if n < 1 or int(rowptr[0]) != 0 or int(rowptr[-1]) != col.numel() or bool((rowptr[1:] < rowptr[:-1]).any()):
            raise ValueError("rowptr must start at 0, never decrease and end at nnz = len(col)")
        if val is not None and val.numel() != col.numel():
            raise ValueError("values and col differ in length")
        row = torch.repeat_interleave(torch.arange(n), rowptr[1:] - rowptr[:-1])
        val = None if val is None else val.cpu()
    elif isinstance(obj, (tuple, list)) or (torch.is_tensor(obj) and not obj.is_sparse and obj.layout == torch.strided):
        ei, val = (obj[0], obj[1]) if isinstance(obj, (tuple, list)) else (obj, None)
        if ei.dim() != 2 or ei.shape[0] != 2 or ei.is_floating_point():
            raise ValueError("edge_index must be an integer tensor of shape [2, E]")
        dev = ei.device
        ei = ei.cpu().long()
        row, col = ei[1], ei[0]
        n = num_nodes if num_nodes is not None else (int(ei.max()) + 1 if ei.numel() else 0)
        val = None if val is None else val.cpu()
    elif torch.is_tensor(obj):
        dev = obj.device
        m = obj.cpu()
        if m.layout != torch.sparse_coo:
            m = m.to_sparse_coo()
        if m.dim() != 2 or m.shape[0] != m.shape[1]:
            raise ValueError(f"the adjacency must be square, got {tuple(m.shape)}")
        m = m.coalesce()
        row, col = m.indices()
        val = m.values()
        n = m.shape[0]
    else:
        try:
            from torch_sparse import SparseTensor       # not installed where this package is tested: this branch is untested
        except ImportError:
            SparseTensor = ()
        if not isinstance(obj, SparseTensor):
            raise TypeError(f"cannot build a graph adjacency from {type(obj).__name__}")
        row, col, val = obj.coo()
        dev = row.device
        row, col = row.cpu(), col.cpu()
        val = None if val is None else val.cpu()
        n = obj.size(0)
    if num_nodes is not None:
        n = int(num_nodes)
    a = _csr_from_coo(row, col, val, n)
    t = _csr_from_coo(col, row, val, n)
    adj = GraphAdjacency(n, *a, *t)
    return adj.to(dev if device is None else device)


# ------------------------------------------------------------------------------------------------ autograd glue
def _propagate(lib, adj, x, x0, h, alpha, p, seed, sid):
    N, C = x.shape
    check(lib.ia_gcn_propagate_fwd(adj.rowptr.data_ptr(), adj.col.data_ptr(), 0, ptr(adj.val), x.data_ptr(), x0.data_ptr(), h.data_ptr(), N, C,
                                   alpha, p, seed, sid, adj.long_rows.data_ptr() if adj.long_rows.numel() else None,
                                   adj.long_rows.numel(), stream_ptr()), "ia_gcn_propagate_fwd")


class GCNEncoderFn(torch.autograd.Function):
    """GCN.forward (reference graph.py:31-44) on the whole graph.  Kept for the backward: x_0, and per layer h and the layer output
    (whose sign is the relu's) -- (2 L + 1) [N, C] fp32 matrices."""

    @staticmethod
    def forward(ctx, anchor, X, enc, adj, training):
        lib = _lib.load()
        N, Fd = X.shape
        C, L = enc.width, len(enc.convs)
        p = float(enc.dropout) if training else 0.0
        seed = Fn.step_seed()
        dev = X.device
        x0 = torch.empty((N, C), device=dev, dtype=F32)
        check(lib.ia_gcn_input_fwd(X.data_ptr(), enc.linear.weight.data_ptr(), enc.linear.bias.data_ptr(), x0.data_ptr(), N, Fd, C, p, seed,
                                   STREAM_INPUT, stream_ptr()), "ia_gcn_input_fwd")
        x, hs, xs = x0, [], []
        for l, conv in enumerate(enc.convs):
            h = torch.empty((N, C), device=dev, dtype=F32)
            _propagate(lib, adj, x, x0, h, conv.alpha, p, seed, STREAM_INPUT + 1 + l)
            out = torch.empty((N, C), device=dev, dtype=F32)
            check(lib.ia_gcn_mix_fwd(h.data_ptr(), conv.weight1.data_ptr(), out.data_ptr(), N, C, conv.beta, p if l == L - 1 else 0.0, seed,
                                     STREAM_INPUT + L + 1, stream_ptr()), "ia_gcn_mix_fwd")
            hs.append(h); xs.append(out)
            x = out
        ctx.enc, ctx.adj, ctx.X, ctx.x0, ctx.hs, ctx.xs, ctx.p, ctx.seed = enc, adj, X, x0, hs, xs, p, seed
        return x

    @staticmethod
    def backward(ctx, dnode):
        lib = _lib.load()
        enc, adj, X, x0, hs, xs, p, seed = ctx.enc, ctx.adj, ctx.X, ctx.x0, ctx.hs, ctx.xs, ctx.p, ctx.seed
        N, Fd = X.shape
        C, L = enc.width, len(enc.convs)
        dev = X.device
        ws_bytes = int(lib.ia_gcn_workspace_bytes(N, C, Fd))
        ws = torch.empty(ws_bytes, device=dev, dtype=torch.uint8)
        d = dnode.contiguous()
        dx0 = torch.empty((N, C), device=dev, dtype=F32)
        lr = adj.long_rows_t
        for l in range(L - 1, -1, -1):
            conv = enc.convs[l]
            dh = torch.empty((N, C), device=dev, dtype=F32)
            wg = conv.weight1.requires_grad
            check(lib.ia_gcn_mix_bwd(d.data_ptr(), xs[l].data_ptr(), hs[l].data_ptr(), conv.weight1.data_ptr(), dh.data_ptr(),
                                     conv.weight1.grad.data_ptr() if wg else None, N, C, conv.beta, p if l == L - 1 else 0.0, ws.data_ptr(),
                                     ws_bytes, stream_ptr()), "ia_gcn_mix_bwd")
            hs[l] = xs[l] = None
            dx = torch.empty((N, C), device=dev, dtype=F32) if l > 0 else None       # layer 1 reads x_0 itself: its dx joins dx0
            check(lib.ia_gcn_propagate_bwd(adj.rowptr_t.data_ptr(), adj.col_t.data_ptr(), 0, ptr(adj.val_t), dh.data_ptr(), ptr(dx),
                                           dx0.data_ptr(), int(l != L - 1), N, C, conv.alpha, p, seed, STREAM_INPUT + 1 + l,
                                           lr.data_ptr() if lr.numel() else None, lr.numel(), stream_ptr()), "ia_gcn_propagate_bwd")
            d = dx
        lin = enc.linear
        if lin.weight.requires_grad:
            check(lib.ia_gcn_input_bwd(dx0.data_ptr(), x0.data_ptr(), X.data_ptr(), lin.weight.grad.data_ptr(), lin.bias.grad.data_ptr(), N, Fd, C,
                                       p, seed, STREAM_INPUT, ws.data_ptr(), ws_bytes, stream_ptr()), "ia_gcn_input_bwd")
        Fn._notify(list(enc.parameters()), final=True)
        ctx.hs = ctx.xs = ctx.x0 = None
        return None, None, None, None, None


class GCNPairGatherFn(torch.autograd.Function):
    """rows idx of the node embeddings under the head's dropout (reference base.py:104,109), fp32 [R, C].  The backward adds the row
    gradients of a node that occurs several times in a fixed order (stable sort by node, one writer per node)."""

    @staticmethod
    def forward(ctx, node, idx, drop_p, stream_id):
        lib = _lib.load()
        N, C = node.shape
        R = idx.numel()
        out = torch.empty((R, C), device=node.device, dtype=F32)
        seed = Fn.step_seed()
        check(lib.ia_gcn_pair_gather_fwd(node.data_ptr(), idx.data_ptr(), out.data_ptr(), R, C, N, drop_p, seed, stream_id, stream_ptr()),
              "ia_gcn_pair_gather_fwd")
        ctx.idx, ctx.shape, ctx.drop, ctx.seed, ctx.stream_id = idx, (N, C), drop_p, seed, stream_id
        return out

    @staticmethod
    def backward(ctx, dout):
        lib = _lib.load()
        N, C = ctx.shape
        dout = dout.contiguous()
        order = torch.argsort(ctx.idx, stable=True).to(torch.int32).contiguous()
        dnode = torch.zeros((N, C), device=dout.device, dtype=F32)
        check(lib.ia_gcn_pair_scatter_bwd(dout.data_ptr(), ctx.idx.data_ptr(), order.data_ptr(), dnode.data_ptr(), ctx.idx.numel(), C, N,
                                          ctx.drop, ctx.seed, ctx.stream_id, stream_ptr()), "ia_gcn_pair_scatter_bwd")
        return dnode, None, None, None


# ------------------------------------------------------------------------------------------------ modules
class GCN2Conv(nn.Module):
    """Parameter holder of torch_geometric.nn.GCN2Conv(channels, alpha, theta, layer, shared_weights=True, normalize=False):
    `weight1` [C, C], glorot-initialised."""

    def __init__(self, channels, alpha, theta=None, layer=None, shared_weights=True, normalize=False):
        super().__init__()
        if not shared_weights or normalize:
            raise ValueError("only shared_weights=True, normalize=False (the reference's arguments) are implemented")
        self.channels, self.alpha = channels, float(alpha)
        self.beta = 1.0 if theta is None or layer is None else math.log(theta / layer + 1)
        self.weight1 = nn.Parameter(torch.empty(channels, channels))
        nn.init.xavier_uniform_(self.weight1)


class GCN(HipModule):
    """reference graph.py:12-44.  forward(x [N, hidden_size] fp32, adj_t) -> node embeddings [N, intermediate_size] fp32."""

    def __init__(self, config):
        super().__init__()
        if config.num_hidden_layers < 1:
            raise ValueError("GCN needs at least one layer")
        C = config.intermediate_size
        if C % 32 or not 32 <= C <= 512:
            raise ValueError(f"intermediate_size {C}: the graph kernels take a multiple of 32 in [32, 512]")
        if config.hidden_size % 4:
            raise ValueError(f"hidden_size (the feature width) {config.hidden_size} must be a multiple of 4")
        self.linear = nn.Linear(config.hidden_size, C)
        self.convs = nn.ModuleList([GCN2Conv(C, config.alpha, config.theta, layer + 1, shared_weights=True, normalize=False)
                                    for layer in range(config.num_hidden_layers)])
        self.dropout = config.hidden_dropout_prob
        self.width = C

    def forward(self, x, adj_t):
        if "anchor" not in self.__dict__:
            self.ensure_arena()
        adj = _adjacency_of(self, adj_t)
        Fn._need_gpu(x, "feature_matrix")
        if not adj.is_cuda:
            raise _lib.ItemAlignError("the adjacency is on the CPU: the MI355X engine has no CPU path (load_adjacency(obj, device='cuda'))")
        if x.dim() != 2 or x.shape[0] != adj.num_nodes or x.shape[1] != self.linear.weight.shape[1]:
            raise ValueError(f"feature_matrix {tuple(x.shape)} does not fit {adj.num_nodes} nodes x {self.linear.weight.shape[1]} features")
        x = x.to(F32).contiguous()
        return GCNEncoderFn.apply(self.anchor, x, self, adj, self.training and torch.is_grad_enabled())


def _adjacency_of(module, obj):
    """The GraphAdjacency of `obj`, converted once per object (the reference hands the same adj_t to every step)."""
    if isinstance(obj, GraphAdjacency):
        return obj
    cache = module.__dict__.get("_adj_cache")
    if cache is None or cache[0] is not obj:
        cache = (obj, load_adjacency(obj))
        module.__dict__["_adj_cache"] = cache
    return cache[1]


class GCNTwoTower(HipModule):
    """reference graph.py:47-132.  forward(feature_matrix, adjacency_matrix, pairs): `pairs` is the list of dicts collate_gnn passes
    through (src_idx, tgt_idx, src_item_id, tgt_item_id, optional item_label as a string)."""

    def __init__(self, config):
        super().__init__()
        if getattr(config, "loss_type", "ce") != "ce":
            raise ValueError(f"loss_type {config.loss_type!r}: the graph model only reaches its loss with 'ce' (quirk G2)")
        self.config = config
        self.num_labels = config.num_labels
        self.encoder = GCN(config)
        self.classifier = TwoTowerClassificationHead(config.intermediate_size, dropout=config.hidden_dropout_prob, num_labels=config.num_labels)
        self.pairwise_loss = os.environ.get("IA_GCN_PAIRWISE_LOSS", "0") == "1"

    def forward(self, feature_matrix, adjacency_matrix, pairs):
        self.ensure_arena()
        if len(pairs) == 0:
            raise ValueError("no pairs")
        node = self.encoder(feature_matrix, adjacency_matrix)
        dev = node.device
        P = len(pairs)
        idx = torch.tensor([int(p["src_idx"]) for p in pairs] + [int(p["tgt_idx"]) for p in pairs], dtype=torch.int32)
        if int(idx.min()) < 0 or int(idx.max()) >= node.shape[0]:
            raise ValueError("pair index outside the graph")
        idx = idx.to(dev)
        have = [p.get("item_label", None) is not None for p in pairs]
        if any(have) and not all(have):
            raise ValueError("either every pair carries an item_label or none does")
        labels = torch.tensor([int(p["item_label"]) for p in pairs], dtype=torch.long, device=dev) if all(have) else None
        train = self.training and torch.is_grad_enabled()
        feats = GCNPairGatherFn.apply(node, idx, float(self.classifier.drop_p) if train else 0.0, STREAM_HEAD)
        src, tgt = feats[:P], feats[P:]
        if self.pairwise_loss:
            _, _, logits, prob, loss = self.classifier(src, tgt, labels=labels)
        else:
            with torch.no_grad():
                _, _, lg_all, prob, _ = self.classifier(src.detach(), tgt.detach())
            logits, loss = lg_all[:1], None
            if labels is not None:      # quirk G1: every label is scored against the logits of pair 0
                _, _, lg0, _, loss = self.classifier(src[:1].expand(P, -1), tgt[:1].expand(P, -1), labels=labels)
                logits = lg0[:1]
        return SequenceClassifierOutput(loss=loss, logits=logits, probs=prob[:, 1], src_embeds=prob[:, 0], tgt_embeds=prob[:, 1])
