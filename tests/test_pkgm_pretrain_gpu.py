"""Knowledge-graph pretraining (pkgm_pretrain.py) on the GPU: one step of PKGM-L2 / PKGM-L1 / TransE-L2 and a 3-step Adam + schedule
trajectory against the reference's own torchkge modules (tests/golden/pkgm_pretrain/*.npz, tools/gen_golden_pkgm_pretrain.py),
run-to-run identical table gradients, the device negative sampler, the CLI end to end into PKGMOneTower, and one step at full size."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from item_alignment_amd.models import kg_pretrain as K

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "pkgm_pretrain")
CASES = ["pkgm_l2", "pkgm_l1", "transe_l2"]
KEYS = {"ent_emb.weight", "rel_emb.weight", "proj_mat.weight"}


def golden(name):
    return np.load(os.path.join(GOLDEN, f"{name}.npz"))


def build(name, z, dev):
    cls = K.PKGMPretrainModel if name.startswith("pkgm") else K.TransEPretrainModel
    m = cls(64, 300, 7, dissimilarity_type="L1" if name.endswith("l1") else "L2")
    m.load_state_dict({k[5:]: torch.from_numpy(z[k]) for k in z.files if k.startswith("init_")})
    m = m.to(dev)
    ids = [torch.from_numpy(z[k]).to(dev) for k in ("h", "t", "r", "nh", "nt")]
    return m, ids


def cos_rel(got, want):
    got, want = got.double().flatten(), want.double().flatten()
    cos = torch.dot(got, want) / (got.norm() * want.norm())
    return cos.item(), ((got - want).norm() / want.norm()).item()


def close_grad(got, want, what):
    cos, rel = cos_rel(got.cpu(), want)
    assert cos >= 0.9999 and rel <= 1e-3, (what, cos, rel)


def grads(m):
    return {k: p.grad.detach().cpu().clone() for k, p in m.named_parameters()}


@pytest.mark.parametrize("name", CASES)
def test_fused_step_matches_the_reference(gpu, name):
    z = golden(name)
    m, ids = build(name, z, gpu)
    loss, pos, neg = m.margin_step(*ids, margin=1.0)
    torch.cuda.synchronize()
    np.testing.assert_allclose(pos.cpu().numpy(), z["pos"], rtol=1e-4, atol=1e-4 * np.abs(z["pos"]).max())
    np.testing.assert_allclose(neg.cpu().numpy(), z["neg"], rtol=1e-4, atol=1e-4 * np.abs(z["neg"]).max())
    assert abs(loss.item() - z["loss"][0]) <= 1e-4 * abs(z["loss"][0])
    g = grads(m)
    assert set(g) == {k[5:] for k in z.files if k.startswith("grad_")}
    for k, v in g.items():
        close_grad(v, torch.from_numpy(z["grad_" + k]), k)


@pytest.mark.parametrize("name", CASES)
def test_autograd_path_matches_the_reference(gpu, name):
    z = golden(name)
    m, ids = build(name, z, gpu)
    pos, neg = m(*ids)
    loss = K.MarginLoss(1.0)(pos, neg)
    loss.backward()
    torch.cuda.synchronize()
    assert abs(loss.item() - z["loss"][0]) <= 1e-4 * abs(z["loss"][0])
    for k, v in grads(m).items():
        close_grad(v, torch.from_numpy(z["grad_" + k]), k)


@pytest.mark.parametrize("name", CASES)
def test_three_step_trajectory_matches_the_reference(gpu, name):
    z = golden(name)
    import json
    meta = json.loads(bytes(z["meta"]).decode())
    m, ids = build(name, z, gpu)
    opt = K.CoupledAdam(m.tables(), lr=meta["lr"], weight_decay=meta["weight_decay"], eps=meta["eps"])
    sched = torch.optim.lr_scheduler.LambdaLR(opt, K.linear_schedule_lambda(meta["warmup_steps"], meta["total_steps"]))
    losses = []
    for _ in range(meta["traj_steps"]):
        opt.zero_grad()
        loss, _, _ = m.margin_step(*ids, margin=meta["margin"])
        opt.step()
        sched.step()
        losses.append(loss.item())
    m.normalize_parameters()
    torch.cuda.synchronize()
    np.testing.assert_allclose(losses, z["traj_losses"], rtol=1e-4)
    for k, v in m.state_dict().items():
        close_grad(v.cpu(), torch.from_numpy(z["traj_" + k]), k)
    for p in m.tables():                                   # the Adam launch left every gradient cleared
        assert p.grad.abs().max().item() == 0.0


def test_table_gradients_are_run_to_run_identical(gpu):
    z = golden("pkgm_l2")
    m, ids = build("pkgm_l2", z, gpu)
    r = ids[2]
    assert 2 * int((r == 0).sum()) > 512                   # relation 0's run spans more than one 512-row piece
    runs = []
    for _ in range(2):
        for p in m.tables():
            p.grad.zero_() if p.grad is not None else None
        m.margin_step(*ids, margin=1.0)
        torch.cuda.synchronize()
        runs.append(grads(m))
    for k in runs[0]:
        assert torch.equal(runs[0][k], runs[1][k]), k
    hot = runs[0]["rel_emb.weight"][0]
    assert hot.abs().max() > 0 and torch.equal(hot, runs[1]["rel_emb.weight"][0])


def test_sampler_ranges_and_bernoulli_fractions(gpu):
    n_ent, n_rel, n = 1000, 5, 1_000_000
    g = torch.Generator().manual_seed(3)
    h = torch.randint(0, n_ent, (n,), generator=g)
    t = torch.randint(0, n_ent, (n,), generator=g)
    r = torch.randint(0, n_rel, (n,), generator=g)
    probs = torch.tensor([0.1, 0.5, 0.9, 0.25, 0.7])
    h, t, r, probs = h.to(gpu), t.to(gpu), r.to(gpu), probs.to(gpu)
    nh, nt = K.corrupt(h, t, r, probs, n_ent, seed=123)
    nh2, nt2 = K.corrupt(h, t, r, probs, n_ent, seed=123)
    assert torch.equal(nh, nh2) and torch.equal(nt, nt2)
    hc, tc = nh != h, nt != t
    assert not (hc & tc).any()                              # never both sides
    head_side = nt == t                                     # head replaced (or the tail draw equal to the original tail: below)
    assert (nh[hc] >= 1).all() and (nh[hc] < n_ent).all() and (nt[tc] >= 1).all() and (nt[tc] < n_ent).all()
    assert (nt[~head_side] >= 1).all()                     # a tail that differs was drawn
    for k in range(n_rel):
        sel = r == k
        cnt = int(sel.sum())
        # a head draw is counted as such; a tail draw equal to its original tail (prob ~ 1 / n_ent) looks like a head draw
        frac = head_side[sel].double().mean().item()
        p = probs[k].item()
        want = p + (1 - p) / (n_ent - 1)
        sigma = (want * (1 - want) / cnt) ** 0.5
        assert abs(frac - want) < 4 * sigma + 1e-9, (k, frac, want, sigma)
    other = K.corrupt(h, t, r, probs, n_ent, seed=124)
    assert not torch.equal(other[0], nh)


def write_kg(d, n_ent=60, n_rel=4, n_facts=600, seed=0):
    rs = np.random.RandomState(seed)
    os.makedirs(d, exist_ok=True)
    with open(os.path.join(d, "train2id.txt"), "w") as f:
        for _ in range(n_facts):
            r = rs.randint(0, n_rel)
            h = rs.randint(0, n_ent // 2)
            f.write(f"{h}\t{r}\t{(h * 7 + r * 3) % n_ent}\n")      # a learnable (h, r) -> t map
    with open(os.path.join(d, "entity2id.txt"), "w") as f:
        f.writelines(f"/item/{i}\t{i}\n" for i in range(n_ent))
    with open(os.path.join(d, "relation2id.txt"), "w") as f:
        f.writelines(f"rel_{i}\t{i}\n" for i in range(n_rel))


def test_cli_end_to_end_into_pkgm_one_tower(gpu, tmp_path):
    data, out = tmp_path / "data", tmp_path / "out"
    write_kg(str(data))
    env = dict(os.environ, PYTHONNOUSERSITE="1")
    res = subprocess.run([sys.executable, os.path.join(ROOT, "pkgm_pretrain.py"), "--data_dir", str(data), "--output_dir", str(out),
                          "--model_name", "pkgm_epoch-{}.bin", "--dim", "64", "--train_batch_size", "128", "--learning_rate", "1e-2",
                          "--num_train_epochs", "6", "--save_epochs", "3", "--log_steps", "2", "--fp16"],
                         capture_output=True, text=True, env=env, timeout=300)
    assert res.returncode == 0, res.stderr[-3000:]
    means = [float(x) for x in re.findall(r"mean loss: ([0-9.]+)", res.stderr + res.stdout)]
    assert len(means) == 6 and means[-1] < means[0], means
    assert "triples/s" in res.stderr + res.stdout
    assert sorted(os.listdir(out)) == ["pkgm_epoch-3.bin", "pkgm_epoch-6.bin"]
    sd = torch.load(out / "pkgm_epoch-6.bin", map_location="cpu")
    assert set(sd) == KEYS
    assert sd["ent_emb.weight"].shape == (60, 64) and sd["rel_emb.weight"].shape == (4, 64) and sd["proj_mat.weight"].shape == (64, 64)
    assert torch.allclose(sd["ent_emb.weight"].norm(dim=1), torch.ones(60), atol=1e-5)     # normalize_parameters() after the epoch

    import item_alignment_amd.models as M
    from bench import roberta_large_config
    from item_alignment_amd.utils import KG_WEIGHTS_NAME, ROBERTA_WEIGHTS_NAME
    S, P, B = 12, 4, 2
    cfg = roberta_large_config(hidden_size=128, num_hidden_layers=2, num_attention_heads=2, intermediate_size=256, interaction_type="one_tower",
                               max_seq_len=S, max_seq_len_pv=None, max_pvs=P, num_entities=60, num_relations=4, kg_embedding_dim=64,
                               entity_projection_bias=False, hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0)
    tower_dir = tmp_path / "tower"
    tower_dir.mkdir()
    torch.manual_seed(5)
    base = M.PKGMOneTower(cfg)
    torch.save({k: v for k, v in base.state_dict().items() if not k.split(".")[-2] in ("ent_emb", "rel_emb", "proj_mat")},
               tower_dir / ROBERTA_WEIGHTS_NAME)
    import shutil
    shutil.copy(out / "pkgm_epoch-6.bin", tower_dir / KG_WEIGHTS_NAME)
    model = M.PKGMOneTower.from_pretrained(str(tower_dir), config=cfg)
    own = model.state_dict()
    for k, v in sd.items():
        tgt = "roberta.embeddings." + k
        assert torch.equal(own[tgt].float(), v), tgt
    model = model.cuda().train()
    rs = np.random.RandomState(1)
    L_ids, L_emb = 2 * (S + P + 1), 2 * (S + 2 * P)
    ids = np.zeros((B, L_ids), np.int64); mask = np.zeros((B, L_emb), np.int64); tt = np.zeros((B, L_emb), np.int64)
    for i in range(B):
        for side in range(2):
            n = int(rs.randint(3, S - 1))
            o_ids, o_emb = side * (S + P + 1), side * (S + 2 * P)
            ids[i, o_ids] = 101 if side == 0 else 102
            ids[i, o_ids + 1:o_ids + 1 + n] = rs.randint(1000, 21128, size=n)
            ids[i, o_ids + 1 + n] = 102
            mask[i, o_emb:o_emb + n + 2] = 1
            ids[i, o_ids + S] = rs.randint(1, 60)
            ids[i, o_ids + S + 1:o_ids + S + 1 + P] = rs.randint(1, 4, size=P)
            mask[i, o_emb + S:o_emb + S + 2 * P] = 1
            tt[i, o_emb:o_emb + S + 2 * P] = side
    pos = np.tile(np.arange(L_emb), (B, 1))
    t = [torch.from_numpy(a).cuda() for a in (ids, mask, tt, pos)]
    o = model(input_ids=t[0], attention_mask=t[1], token_type_ids=t[2], position_ids=t[3], labels=torch.tensor([1, 0]).cuda())
    model.param_arena.zero_grad()
    o.loss.backward()
    model.param_arena.adamw_step(1e-4)
    torch.cuda.synchronize()
    assert torch.isfinite(o.loss).item() and torch.isfinite(model.param_arena.master).all().item()


def test_full_size_step_and_normalise(gpu):
    import time
    n_ent, n_rel, D, B = 258211, 1379, 1024, 32768
    torch.manual_seed(0)
    m = K.PKGMPretrainModel(D, n_ent, n_rel).to(gpu)
    opt = K.CoupledAdam(m.tables(), lr=1e-4, weight_decay=1e-5)
    g = torch.Generator(device=gpu).manual_seed(1)
    h = torch.randint(0, n_ent, (B,), device=gpu, generator=g)
    t = torch.randint(0, n_ent, (B,), device=gpu, generator=g)
    r = torch.randint(0, n_rel, (B,), device=gpu, generator=g)
    probs = torch.full((n_rel,), 0.5, device=gpu)
    nh, nt = K.corrupt(h, t, r, probs, n_ent, seed=9)
    times = []
    for _ in range(2):
        t0 = time.perf_counter()
        opt.zero_grad()
        loss, pos, neg = m.margin_step(h, t, r, nh, nt, margin=1.0)
        opt.step()
        torch.cuda.synchronize()
        times.append(time.perf_counter() - t0)
    m.normalize_parameters()
    torch.cuda.synchronize()
    assert torch.isfinite(loss).all() and torch.isfinite(pos).all() and torch.isfinite(neg).all()
    for p in m.tables():
        assert torch.isfinite(p).all().item()
    norms = m.ent_emb.weight.norm(dim=1)
    assert (norms - 1).abs().max().item() < 1e-4
    assert times[-1] < 5.0, times                             # one step, warm
