"""Writes tests/golden/gcn/gcn_two_tower.npz from the reference's own graph model.

    python tools/gen_golden_gcn.py <reference checkout>

The reference's src/models/graph.py (GCN, GCNTwoTower: the wrapper, the per-pair loop and its first-pair-only logits, quirk G1) is
imported under the stub recipe of SURVEY.md Appendix B (oracle/ref_harness.py), with the stub torch_geometric.nn.GCN2Conv replaced
by the layer restated from its published definition -- torch_geometric itself cannot be installed, so only that layer is not the
reference's code ("parity unpinned by PyG").  A 300-node graph, F = 64, C = 32, L = 3, 8 pairs that share nodes,
eval mode, fp32 on the CPU: inputs, seeded weights, node embeddings, loss / logits / probs / src_embeds / tgt_embeds, the gradient of
every parameter, and the weights after 3 steps of the reference's optimiser (torch AdamW, two parameter groups, betas (0.9, 0.98))
under get_linear_schedule_with_warmup(1, 10).  The file is byte-reproducible.
"""
import io
import math
import os
import sys
import types
import zipfile
from types import SimpleNamespace

import numpy as np
import torch
from torch import nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden", "gcn")


class GCN2Conv(nn.Module):
    """torch_geometric.nn.GCN2Conv restated (shared_weights=True, normalize=False): out = (1 - beta) h + beta h W1,
    h = (1 - alpha) adj_t @ x + alpha x_0, beta = log(theta / layer + 1)."""

    def __init__(self, channels, alpha, theta=None, layer=None, shared_weights=True, cached=False, add_self_loops=True, normalize=True):
        super().__init__()
        assert shared_weights and not normalize
        self.alpha = alpha
        self.beta = 1.0 if theta is None or layer is None else math.log(theta / layer + 1)
        self.weight1 = nn.Parameter(torch.empty(channels, channels))
        nn.init.xavier_uniform_(self.weight1)

    def forward(self, x, x_0, adj_t):
        h = torch.sparse.mm(adj_t, x) * (1 - self.alpha) + self.alpha * x_0
        return torch.addmm(h, h, self.weight1, beta=1 - self.beta, alpha=self.beta)


def write_npz(path, arrays):
    """np.savez with a fixed timestamp per member (zipfile stamps the current time otherwise)."""
    with zipfile.ZipFile(path, "w", compression=zipfile.ZIP_DEFLATED) as zf:
        for k in sorted(arrays):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.ascontiguousarray(arrays[k]), allow_pickle=False)
            info = zipfile.ZipInfo(k + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.external_attr = 0o644 << 16
            info.compress_type = zipfile.ZIP_DEFLATED
            zf.writestr(info, buf.getvalue())


def main(reference):
    sys.path.insert(0, ROOT)
    from oracle import ref_harness
    ref_harness.REFERENCE_ROOT = reference
    import transformers  # noqa: F401  (before the stubs, as in ref_harness)
    pyg, pyg_nn = types.ModuleType("torch_geometric"), types.ModuleType("torch_geometric.nn")
    pyg.__path__, pyg_nn.__path__ = [], []
    pyg_nn.GCN2Conv = GCN2Conv
    pyg.nn = pyg_nn
    sys.modules["torch_geometric"], sys.modules["torch_geometric.nn"] = pyg, pyg_nn
    ref_harness.load_reference()
    import src.models.graph as G
    G.SequenceClassifierOutput = sys.modules["src.models.base"].SequenceClassifierOutput
    from transformers import get_linear_schedule_with_warmup

    torch.use_deterministic_algorithms(True)
    torch.manual_seed(20221016)
    rs = np.random.RandomState(20221016)
    N, F, C, L = 300, 64, 32, 3
    X = torch.from_numpy(rs.standard_normal((N, F)).astype(np.float32))
    e = np.unique(rs.randint(0, N, size=(2, 5 * N)), axis=1)                # unsymmetric, no duplicate edges
    e = e[:, e[1] != 17]                                                    # node 17 has no in-edges: an empty row of A
    ei = torch.from_numpy(e)
    adj_t = torch.sparse_coo_tensor(torch.stack((ei[1], ei[0])), torch.ones(ei.shape[1]), (N, N)).coalesce()
    src, tgt, labels = [3, 7, 3, 50, 120, 7, 299, 17], [9, 3, 9, 60, 7, 200, 1, 2], [1, 0, 1, 1, 0, 0, 1, 0]
    pairs = [{"src_idx": s, "tgt_idx": t, "src_item_id": str(s), "tgt_item_id": str(t), "item_label": str(y)} for s, t, y in zip(src, tgt, labels)]
    cfg = SimpleNamespace(hidden_size=F, intermediate_size=C, num_hidden_layers=L, hidden_dropout_prob=0.1, num_labels=2, alpha=0.1, theta=0.5,
                          loss_type="ce")
    model = G.GCNTwoTower(cfg).eval()
    arrays = {"N": np.int64(N), "F": np.int64(F), "C": np.int64(C), "L": np.int64(L), "X": X.numpy(), "edge_index": ei.numpy().astype(np.int64),
              "src": np.asarray(src, np.int64), "tgt": np.asarray(tgt, np.int64), "labels": np.asarray(labels, np.int64)}
    for k, v in model.state_dict().items():
        arrays["w." + k] = v.detach().numpy().copy()
    with torch.no_grad():
        arrays["node"] = model.encoder(X, adj_t).numpy()
    out = model(X, adj_t, pairs)
    for k in ("loss", "logits", "probs", "src_embeds", "tgt_embeds"):
        arrays["literal." + k] = getattr(out, k).detach().numpy().copy()
    model.zero_grad()
    out.loss.backward()
    for k, p in model.named_parameters():
        arrays["literal.grad." + k] = p.grad.detach().numpy().copy()
    no_decay = ["bias", "LayerNorm.weight"]
    groups = [{"params": [p for n, p in model.named_parameters() if not any(nd in n for nd in no_decay)], "weight_decay": 1e-5},
              {"params": [p for n, p in model.named_parameters() if any(nd in n for nd in no_decay)], "weight_decay": 0.0}]
    opt = torch.optim.AdamW(groups, lr=1e-3, eps=1e-8, betas=(0.9, 0.98))
    sched = get_linear_schedule_with_warmup(opt, 1, 10)
    for _ in range(3):
        opt.zero_grad()
        model(X, adj_t, pairs).loss.backward()
        opt.step()
        sched.step()
    for k, p in model.named_parameters():
        arrays["after3.literal." + k] = p.detach().numpy().copy()
    os.makedirs(OUT, exist_ok=True)
    write_npz(os.path.join(OUT, "gcn_two_tower.npz"), arrays)
    print("wrote", os.path.join(OUT, "gcn_two_tower.npz"), {k: getattr(v, "shape", ()) for k, v in arrays.items() if k.startswith("literal.")})


if __name__ == "__main__":
    if len(sys.argv) != 2:
        raise SystemExit(__doc__)
    main(sys.argv[1])
