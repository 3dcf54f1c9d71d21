"""Host side of the knowledge-graph pretraining job (pkgm_pretrain.py): Bernoulli probabilities, data loading, the learning-rate
schedule, the gradient-accumulation quirk, the Xavier + normalise initialisation and the CLI's refusals (no GPU needed)."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from item_alignment_amd.models import kg_pretrain as K

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "pkgm_pretrain")


def golden(name):
    return np.load(os.path.join(GOLDEN, f"{name}.npz"))


def test_bernoulli_probs_equal_the_reference():
    z = golden("pkgm_l2")
    kg = K.KnowledgeGraph(*(torch.from_numpy(z[k]) for k in ("h", "t", "r")), 300, 7)
    got = K.bernoulli_probs(kg)
    assert got.dtype == torch.float32
    assert np.array_equal(got.numpy(), z["bern_probs"])


def test_bernoulli_probs_unseen_relation_is_one_half():
    kg = K.KnowledgeGraph(torch.tensor([0, 0, 1]), torch.tensor([1, 2, 2]), torch.tensor([0, 0, 0]), 3, 3)
    p = K.bernoulli_probs(kg)
    assert p[1] == 0.5 and p[2] == 0.5
    # relation 0: 2 tails per head (tph = 3 / 2), 1.5 heads per tail (hpt = 3 / 2) -> 0.5; then a skewed one
    kg = K.KnowledgeGraph(torch.tensor([0, 0, 0]), torch.tensor([1, 2, 3]), torch.tensor([0, 0, 0]), 4, 1)
    assert K.bernoulli_probs(kg)[0].item() == pytest.approx(3.0 / 4.0)


@pytest.mark.parametrize("name", ["pkgm_l2", "pkgm_l1", "transe_l2"])
def test_initialisation_matches_the_reference_rng_order(name):
    z = golden(name)
    cls = K.PKGMPretrainModel if name.startswith("pkgm") else K.TransEPretrainModel
    torch.manual_seed(11)
    m = cls(64, 300, 7, dissimilarity_type="L1" if name.endswith("l1") else "L2")
    sd = m.state_dict()
    want = sorted(k[5:] for k in z.files if k.startswith("init_"))
    assert sorted(sd) == want
    for k in want:
        assert np.array_equal(sd[k].numpy(), z["init_" + k]), k


def test_torus_norms_are_rejected():
    with pytest.raises(ValueError, match="torus"):
        K.PKGMPretrainModel(8, 4, 2, dissimilarity_type="torus_L2")


def write_kg(d, facts, n_ent, n_rel):
    with open(os.path.join(d, "train2id.txt"), "w") as f:
        for h, r, t in facts:
            f.write(f"{h}\t{r}\t{t}\n")
    with open(os.path.join(d, "entity2id.txt"), "w") as f:
        for i in range(n_ent):
            f.write(f"/item/{i}\t{i}\n")
    with open(os.path.join(d, "relation2id.txt"), "w") as f:
        for i in range(n_rel):
            f.write(f"rel_{i}\t{i}\n")


def test_load_ccks_uses_the_written_ids(tmp_path):
    write_kg(tmp_path, [(3, 0, 5), (0, 1, 9), (7, 0, 3)], n_ent=12, n_rel=2)
    kg = K.load_ccks(str(tmp_path))
    assert (kg.n_ent, kg.n_rel, len(kg)) == (12, 2, 3)
    assert kg.head_idx.tolist() == [3, 0, 7] and kg.relations.tolist() == [0, 1, 0] and kg.tail_idx.tolist() == [5, 9, 3]
    assert kg.head_idx.dtype == torch.int64


def test_load_ccks_rejects_ids_outside_the_id_files(tmp_path):
    write_kg(tmp_path, [(3, 0, 12)], n_ent=12, n_rel=2)
    with pytest.raises(ValueError, match="'to'"):
        K.load_ccks(str(tmp_path))


def test_schedule_counts_and_lr_sequence():
    # pkgm_pretrain.py: int(len(kg) / bs / gas) * (epochs - start_epoch), warm-up int(total * proportion)
    assert K.schedule_steps(100_000, 32768, 1, 2000, 0, 0.2) == (3 * 2000, 1200)
    assert K.schedule_steps(100_000, 32768, 2, 10, 4, 0.2) == (6, 1)
    total, warm = K.schedule_steps(1000, 100, 1, 3, 0, 0.2)
    assert (total, warm) == (30, 6)
    opt = torch.optim.SGD([torch.nn.Parameter(torch.zeros(1))], lr=1e-3)
    sched = torch.optim.lr_scheduler.LambdaLR(opt, K.linear_schedule_lambda(warm, total))
    lrs = []
    for _ in range(total + 2):
        lrs.append(opt.param_groups[0]["lr"])
        opt.step()
        sched.step()
    want = [1e-3 * (s / warm if s < warm else max(0.0, (total - s) / (total - warm))) for s in range(total + 2)]
    assert lrs == pytest.approx(want, abs=1e-12)
    assert lrs[0] == 0.0 and lrs[warm] == pytest.approx(1e-3)


def test_accumulation_quirk_only_every_kth_batch_steps():
    assert K.n_batches(10, 3) == 4 and K.n_batches(9, 3) == 3
    assert K.stepping_batches(7, 1) == list(range(7))
    assert K.stepping_batches(7, 3) == [2, 5]          # batch 6 is computed and dropped; batches 0, 1, 3, 4 are cleared unused


def run_cli(*args):
    env = dict(os.environ, PYTHONNOUSERSITE="1")
    return subprocess.run([sys.executable, os.path.join(ROOT, "pkgm_pretrain.py"), *args], capture_output=True, text=True, env=env,
                          timeout=120)


@pytest.mark.parametrize("extra,msg", [(["--norm", "torus_L2"], "torus"), (["--norm", "torus_L1"], "torus"), (["--do_test"], "do_test"),
                                       (["--do_eval"], "do_eval"), (["--model_name", "distmult_{}.bin"], "Unsuported model name")])
def test_cli_rejects_what_is_not_built(tmp_path, extra, msg):
    write_kg(tmp_path, [(1, 0, 2)], n_ent=4, n_rel=1)
    res = run_cli("--data_dir", str(tmp_path), "--output_dir", str(tmp_path / "out"), "--model_name", "pkgm_epoch-{}.bin", *extra)
    assert res.returncode != 0
    assert msg in res.stderr
    assert not (tmp_path / "out").exists()


# ------------------------------------------------------------------------- the fp64 reference of tests/kgpt_reference.py, pinned
# to torchkge's own fp32 results (the goldens), before the GPU tests use it at shapes where no golden exists
import kgpt_reference as R  # noqa: E402

TAU_GOLDEN = 1e-5


def golden_case(name):
    import json
    z = golden(name)
    meta = json.loads(bytes(z["meta"]).decode())
    t = {k: torch.from_numpy(z[k]) for k in z.files if k != "meta"}
    proj = t.get("init_proj_mat.weight")
    return z, meta, t, proj


def within(got, ref, S, tau, U=None):
    """max over elements of (|got - ref| - U) / (tau * S): the share of the bound tau * S used (<= 1 inside it); an element with
    S == 0 must match exactly."""
    err = (got.double() - ref).abs() - (0 if U is None else U)
    assert (err[S == 0] <= 0).all()
    return (err.clamp_min(0) / (tau * torch.where(S > 0, S, torch.ones_like(S)))).max().item()


@pytest.mark.parametrize("name", ["pkgm_l2", "pkgm_l1", "transe_l2"])
def test_fp64_reference_reproduces_the_torchkge_step(name):
    z, meta, t, proj = golden_case(name)
    norm = 1 if meta["norm"] == "L1" else 2
    ref = R.score_step(t["init_ent_emb.weight"], t["init_rel_emb.weight"], proj, t["h"], t["t"], t["r"], t["nh"], t["nt"], norm,
                       margin=meta["margin"], sign_tol=True)
    assert within(t["pos"], ref["pos"], ref["S_pos"], TAU_GOLDEN) <= 1.0
    assert within(t["neg"], ref["neg"], ref["S_neg"], TAU_GOLDEN) <= 1.0
    assert (meta["margin"] - ref["pos"] + ref["neg"]).abs().min() > 1e-4          # no hinge decision near a tie
    assert abs(float(t["loss"][0]) - ref["loss"].item()) <= TAU_GOLDEN * (ref["S_pos"] + ref["S_neg"]).sum().item()
    for key, g in (("ent_emb.weight", "ent"), ("rel_emb.weight", "rel"), ("proj_mat.weight", "proj")):
        if proj is None and g == "proj":
            continue
        q = within(t["grad_" + key], ref["grad_" + g], ref["S_" + g], TAU_GOLDEN, ref["U_" + g])
        assert q <= 1.0 / 4, (key, q)                                                 # torchkge's fp32 within tau / 4 * S
    # the rows the golden's step never touched have exactly zero gradient in both
    untouched = ref["count_ent"] == 0
    assert untouched.any() and (t["grad_ent_emb.weight"][untouched] == 0).all() and (ref["grad_ent"][untouched] == 0).all()


@pytest.mark.parametrize("name", ["pkgm_l2", "pkgm_l1", "transe_l2"])
def test_fp64_reference_reproduces_the_torchkge_trajectory(name):
    """3 x (step, coupled-L2 Adam, LambdaLR) and normalize_parameters() in fp64 against torchkge + torch.optim.Adam in fp32."""
    z, meta, t, proj = golden_case(name)
    norm = 1 if meta["norm"] == "L1" else 2
    tabs = {"ent_emb.weight": t["init_ent_emb.weight"].double(), "rel_emb.weight": t["init_rel_emb.weight"].double()}
    if proj is not None:
        tabs["proj_mat.weight"] = proj.double()
    state = {k: (torch.zeros_like(v), torch.zeros_like(v)) for k, v in tabs.items()}
    lam = K.linear_schedule_lambda(meta["warmup_steps"], meta["total_steps"])
    losses = []
    for step in range(meta["traj_steps"]):
        ref = R.score_step(tabs["ent_emb.weight"], tabs["rel_emb.weight"], tabs.get("proj_mat.weight"), t["h"], t["t"], t["r"], t["nh"],
                           t["nt"], norm, margin=meta["margin"])
        losses.append(ref["loss"].item())
        for k, g in (("ent_emb.weight", "ent"), ("rel_emb.weight", "rel"), ("proj_mat.weight", "proj")):
            if k not in tabs:
                continue
            m, v = state[k]
            p, m, v, *_ = R.adam_l2(tabs[k], m, v, [ref["grad_" + g]], [meta["lr"] * lam(step)], eps=meta["eps"],
                                    weight_decay=meta["weight_decay"], first_step=step + 1)
            tabs[k], state[k] = p, (m, v)
    tabs["ent_emb.weight"] = R.row_normalize(tabs["ent_emb.weight"])
    np.testing.assert_allclose(losses, z["traj_losses"], rtol=1e-5)
    for k, v in tabs.items():
        got = torch.from_numpy(z["traj_" + k]).double()
        assert (got - v).abs().max().item() <= 2e-5 * v.abs().max().item(), k


def test_fp64_adam_reference_is_torch_adam():
    """R.adam_l2 against torch.optim.Adam(foreach=False) run in fp64: the same formula, to fp64 rounding."""
    g = torch.Generator().manual_seed(4)
    p0 = torch.randn(37, generator=g, dtype=torch.float64)
    grads = [torch.randn(37, generator=g, dtype=torch.float64) for _ in range(10)]
    lrs = [1e-2 * (1 + 0.3 * i) for i in range(10)]
    for wd in (0.0, 1e-5, 1e-2):
        p = torch.nn.Parameter(p0.clone())
        opt = torch.optim.Adam([p], lr=lrs[0], weight_decay=wd, foreach=False)
        for gr, lr in zip(grads, lrs):
            opt.param_groups[0]["lr"] = lr
            p.grad = gr.clone()
            opt.step()
        want, m, v, *_ = R.adam_l2(p0, torch.zeros(37, dtype=torch.float64), torch.zeros(37, dtype=torch.float64), grads, lrs, weight_decay=wd)
        assert torch.allclose(p.detach(), want, rtol=1e-13, atol=1e-15), wd
        assert torch.allclose(opt.state[p]["exp_avg"], m, rtol=1e-13, atol=1e-15)
        assert torch.allclose(opt.state[p]["exp_avg_sq"], v, rtol=1e-13, atol=1e-15)


def test_fp64_row_normalize_reference():
    x = torch.tensor([[3.0, 4.0], [0.0, 0.0], [1e-13, 0.0]], dtype=torch.float64)
    y = R.row_normalize(x)
    assert y.dtype == torch.float64
    assert torch.equal(y[0], torch.tensor([0.6, 0.8], dtype=torch.float64)) and (y[1] == 0).all()
    assert y[2, 0].item() == pytest.approx(0.1, rel=1e-12)                 # below eps: divided by 1e-12, as F.normalize does
