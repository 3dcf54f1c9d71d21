"""TEST INFRASTRUCTURE -- golden vectors of the knowledge-graph pretraining job (reference pkgm_pretrain.py) captured from the
reference's own torchkge modules on CPU: writes tests/golden/pkgm_pretrain/{pkgm_l2,pkgm_l1,transe_l2}.npz
(a folder of their own: every top-level tests/golden/*.npz is an oracle case of tests/test_oracle_golden.py).

    python tools/gen_golden_pkgm_pretrain.py <reference checkout>

Each file holds a small KG (300 entities, 7 relations, 512 facts; relation 0 owns 350 facts = 700 of the 1024 relation-gradient
contributions, so its run crosses the 512-row pieces of the segment sum), one fixed set of Bernoulli negatives, the initial
weights, pos / neg / loss and the three gradients of one step, the weights after 3 Adam + LambdaLR steps (weight_decay 1e-5) and
an end-of-epoch normalize_parameters(), and bern_probs.  Re-running reproduces the files byte for byte.
"""
import io
import json
import os
import sys
import zipfile

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden", "pkgm_pretrain")

N_ENT, N_REL, N_FACTS, DIM = 300, 7, 512, 64
MARGIN, LR, WD, EPS = 1.0, 1e-2, 1e-5, 1e-8
TOTAL_STEPS, WARMUP_STEPS, TRAJ_STEPS = 10, 1, 3
CASES = {"pkgm_l2": ("PKGMModel", "L2"), "pkgm_l1": ("PKGMModel", "L1"), "transe_l2": ("TransEModel", "L2")}


def make_kg():
    g = np.random.default_rng(20261015)
    # exactly 350 facts of relation 0, in scattered file positions
    idx0 = g.permutation(N_FACTS)[:350]
    r = g.integers(1, N_REL, N_FACTS)
    r[idx0] = 0
    h = g.integers(0, N_ENT, N_FACTS)
    t = g.integers(0, N_ENT, N_FACTS)
    h[r == 0] = g.integers(0, 40, int((r == 0).sum()))          # a many-to-many hot relation with repeated heads
    return h.astype(np.int64), t.astype(np.int64), r.astype(np.int64)


def write_npz(path, arrays):
    """np.savez with a fixed timestamp per member (zipfile stamps the current time otherwise)."""
    with zipfile.ZipFile(path, "w", compression=zipfile.ZIP_STORED) as zf:
        for k in sorted(arrays):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.ascontiguousarray(arrays[k]), allow_pickle=False)
            info = zipfile.ZipInfo(k + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.external_attr = 0o644 << 16
            zf.writestr(info, buf.getvalue())


def main(reference):
    sys.path.insert(0, os.path.join(reference, "torchkge"))
    from torchkge.data_structures import KnowledgeGraph
    from torchkge.models import translation as T
    from torchkge.sampling import BernoulliNegativeSampler
    from torchkge.utils.losses import MarginLoss
    import pandas as pd

    torch.use_deterministic_algorithms(True)
    os.makedirs(OUT, exist_ok=True)
    h, t, r = make_kg()
    df = pd.DataFrame({"from": h, "rel": r, "to": t})
    kg = KnowledgeGraph(df=df, ent2ix={i: i for i in range(N_ENT)}, rel2ix={i: i for i in range(N_REL)})
    torch.manual_seed(7)
    sampler = BernoulliNegativeSampler(kg)
    nh, nt = sampler.corrupt_batch(kg.head_idx, kg.tail_idx, kg.relations, n_neg=1)
    heads, tails, rels = kg.head_idx, kg.tail_idx, kg.relations
    for name, (cls_name, norm) in CASES.items():
        torch.manual_seed(11)
        model = getattr(T, cls_name)(DIM, N_ENT, N_REL, dissimilarity_type=norm)
        keys = list(model.state_dict())
        init = {k: v.detach().clone() for k, v in model.state_dict().items()}
        crit = MarginLoss(MARGIN)
        pos, neg = model(heads, tails, rels, nh, nt)
        loss = crit(pos, neg)
        loss.backward()
        out = {"h": h, "t": t, "r": r, "nh": nh.numpy(), "nt": nt.numpy(), "bern_probs": sampler.bern_probs.numpy(),
               "pos": pos.detach().numpy(), "neg": neg.detach().numpy(), "loss": np.array([loss.item()], np.float32)}
        for k in keys:
            out["init_" + k] = init[k].numpy()
            out["grad_" + k] = dict(model.named_parameters())[k].grad.numpy().copy()
        # 3 steps of the trainer: zero_grad, forward, loss, backward, Adam (coupled L2), LambdaLR; then normalize_parameters()
        opt = torch.optim.Adam(model.parameters(), lr=LR, weight_decay=WD, eps=EPS)

        def lr_lambda(step):
            if step < WARMUP_STEPS:
                return float(step) / float(max(1, WARMUP_STEPS))
            return max(0.0, float(TOTAL_STEPS - step) / float(max(1, TOTAL_STEPS - WARMUP_STEPS)))
        sched = torch.optim.lr_scheduler.LambdaLR(opt, lr_lambda)
        losses = []
        for _ in range(TRAJ_STEPS):
            opt.zero_grad()
            p, n = model(heads, tails, rels, nh, nt)
            ls = crit(p, n)
            ls.backward()
            opt.step()
            sched.step()
            losses.append(ls.item())
        model.normalize_parameters()
        for k, v in model.state_dict().items():
            out["traj_" + k] = v.numpy()
        out["traj_losses"] = np.array(losses, np.float32)
        out["meta"] = np.frombuffer(json.dumps(dict(model=cls_name, norm=norm, n_ent=N_ENT, n_rel=N_REL, dim=DIM, margin=MARGIN, lr=LR,
                                                    weight_decay=WD, eps=EPS, total_steps=TOTAL_STEPS, warmup_steps=WARMUP_STEPS,
                                                    traj_steps=TRAJ_STEPS, init_seed=11, keys=keys), sort_keys=True).encode(), np.uint8)
        write_npz(os.path.join(OUT, f"{name}.npz"), out)
        print(name, "loss", loss.item(), "after", losses)


if __name__ == "__main__":
    if len(sys.argv) != 2:
        raise SystemExit(__doc__)
    main(sys.argv[1])
