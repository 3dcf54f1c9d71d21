"""Link-prediction ranking on the device (ia_kgpt_lp_rank, the LinkPredictionEvaluator of pkgm_pretrain.py --do_eval / --do_test)
against the torchkge goldens, the fp64 rank bracket of tests/linkpred_reference.py, exact integer grids and the CLI end to end."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from item_alignment_amd import _lib
from item_alignment_amd.models import kg_pretrain as K

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import linkpred_reference as LR  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden", "pkgm_pretrain")
CASES = ["pkgm_l2", "pkgm_l1", "transe_l2"]
RUNS = [("t", "test", ("train", "test")), ("vt", "test", ("train", "valid", "test")), ("vv", "valid", ("train", "valid", "test"))]
DEV = "cuda"
pytestmark = pytest.mark.gpu


def golden(name):
    return np.load(os.path.join(GOLDEN, f"linkpred_{name}.npz"))


def kg_of(z, split):
    return K.KnowledgeGraph(*(torch.from_numpy(z[f"{split}_{c}"]) for c in ("h", "t", "r")), 300, 8)


def model_of(z, name):
    cls = K.PKGMPretrainModel if name.startswith("pkgm") else K.TransEPretrainModel
    m = cls(64, 300, 8, dissimilarity_type="L1" if name.endswith("l1") else "L2")
    m.load_state_dict({k[3:]: torch.from_numpy(z[k]) for k in z.files if k.startswith("sd_")})
    return m.to(DEV)


@pytest.mark.gpu
@pytest.mark.parametrize("name", CASES)
@pytest.mark.parametrize("prefix,split,loaded", RUNS)
def test_ranks_equal_torchkge(gpu, name, prefix, split, loaded):
    z = golden(name)
    norm = 1 if name.endswith("l1") else 2
    f = K.KGFilters.build([kg_of(z, s) for s in loaded])
    ev = K.LinkPredictionEvaluator(model_of(z, name), kg_of(z, split), f)
    ev.evaluate(17)
    ent, rel = torch.from_numpy(z["sd_ent_emb.weight"]), torch.from_numpy(z["sd_rel_emb.weight"])
    h, t, r = (torch.from_numpy(z[f"{split}_{c}"]) for c in ("h", "t", "r"))
    for side, sname, groups, anchor in ((LR.TAIL, "tails", f.tails, h), (LR.HEAD, "heads", f.heads, t)):
        near = torch.from_numpy(z[f"near_tie_{split}_{sname}"])
        got = {"rank": getattr(ev, f"rank_true_{sname}"), "filt": getattr(ev, f"filt_rank_true_{sname}")}
        s, S = LR.scores_fp64(ent, rel, h, t, r, norm, side)
        true = LR.true_ids(h, t, side)
        mask = LR.filter_mask(groups, groups.group_of(anchor.numpy(), r.numpy()), 300)
        for kind, fm in (("rank", None), ("filt", mask)):
            g = got[kind]
            assert g.dtype == torch.int64 and g.device.type == "cpu"
            want = torch.from_numpy(z[f"{prefix}_{kind}_{sname}"])
            # the contract: exact where no candidate is within 1e-4 S of the true score, inside the fp64 bracket everywhere
            assert torch.equal(g[~near], want[~near]), (sname, kind)
            lo, hi = LR.bracket(s, S, true, fm)
            assert bool(((g >= lo) & (g <= hi)).all()), (sname, kind)
            # these fixed fixtures: the near ties come out as torchkge's too (the fp32 direct difference form rounds alike there)
            assert torch.equal(g[near], want[near]), (sname, kind, "near ties")
    assert ev.results_text() == bytes(z[f"{prefix}_text"]).decode()


def rand_tables(g, n_ent, n_rel, D, scale=True):
    ent = torch.randn(n_ent, D, generator=g)
    if scale:
        ent *= torch.rand(n_ent, 1, generator=g) * 1.5 + 0.5
    rel = torch.randn(n_rel, D, generator=g) * 0.3
    return ent.to(DEV), rel.to(DEV)


def rand_filter(g, h, t, r, n_ent, big=False):
    """Groups over the queries' own facts plus random extra facts; big: one (h0, r0) key with 30 000 members."""
    extra = 3 * len(h)
    eh = h[torch.randint(0, len(h), (extra,), generator=g)]
    er = r[torch.randint(0, len(h), (extra,), generator=g)]
    et = torch.randint(0, n_ent, (extra,), generator=g)
    hs, ts, rs = [h, eh], [t, et], [r, er]
    if big:
        m = torch.randperm(n_ent, generator=g)[:30000]
        hs.append(torch.full((30000,), int(h[0]))), ts.append(m), rs.append(torch.full((30000,), int(r[0])))
        hs.append(m), ts.append(torch.full((30000,), int(t[0]))), rs.append(torch.full((30000,), int(r[0])))
    kg = K.KnowledgeGraph(torch.cat(hs), torch.cat(ts), torch.cat(rs), n_ent, int(r.max()) + 1)
    return K.KGFilters.build([kg])


def check_bracket(ent, rel, h, t, r, norm, side, f, rk, fr):
    groups = f.tails if side == LR.TAIL else f.heads
    anchor = h if side == LR.TAIL else t
    qg = groups.group_of(anchor.numpy(), r.numpy())
    s, S = LR.scores_fp64(ent, rel, h.to(DEV), t.to(DEV), r.to(DEV), norm, side)
    true = LR.true_ids(h, t, side).to(DEV)
    mask = LR.filter_mask(groups, qg, ent.shape[0], device=DEV)
    for got, fm in ((rk, None), (fr, mask)):
        lo, hi = LR.bracket(s, S, true, fm)
        bad = ((got.to(DEV) < lo) | (got.to(DEV) > hi)).nonzero()
        assert bad.numel() == 0, (bad[:4].tolist(), got.to(DEV)[bad[:4, 0]].tolist(), lo[bad[:4, 0]].tolist(), hi[bad[:4, 0]].tolist())
    assert bool((fr >= 1).all() and (fr <= rk).all())


SWEEP = [(4, 1, 1), (8, 2, 7), (60, 63, 256), (764, 64, 7), (768, 65, 256), (1028, 1000, 4099), (60, 40001, 256), (8, 40001, 7)]


@pytest.mark.gpu
@pytest.mark.parametrize("D,n_ent,B", SWEEP)
@pytest.mark.parametrize("norm", [1, 2])
def test_ranks_lie_in_the_fp64_bracket(gpu, D, n_ent, B, norm):
    g = torch.Generator().manual_seed(D * 7 + n_ent + B + norm)
    n_rel = 5
    ent, rel = rand_tables(g, n_ent, n_rel, D)
    h, t, r = torch.randint(0, n_ent, (B,), generator=g), torch.randint(0, n_ent, (B,), generator=g), torch.randint(0, n_rel, (B,), generator=g)
    f = rand_filter(g, h, t, r, n_ent, big=n_ent > 30000)
    for side, groups, anchor in ((LR.TAIL, f.tails, h), (LR.HEAD, f.heads, t)):
        qg = groups.group_of(anchor.numpy(), r.numpy())
        rk, fr = K.lp_rank(ent, rel, h, t, r, norm, side, groups, qg)
        torch.cuda.synchronize()
        check_bracket(ent, rel, h, t, r, norm, side, f, rk, fr)


@pytest.mark.gpu
@pytest.mark.parametrize("D,n_ent,B", [(60, 1000, 300), (1028, 700, 130), (8, 40001, 7)])
@pytest.mark.parametrize("norm", [1, 2])
def test_scores_and_ranks_are_self_consistent(gpu, D, n_ent, B, norm):
    """The ranks equal the counts over the scores the same call stored (pins the scan and the listed mode to the same bits), the
    scores are within tau S of fp64, and a call without scores returns the same ranks."""
    g = torch.Generator().manual_seed(B + D)
    ent, rel = rand_tables(g, n_ent, 3, D)
    h, t, r = torch.randint(0, n_ent, (B,), generator=g), torch.randint(0, n_ent, (B,), generator=g), torch.randint(0, 3, (B,), generator=g)
    f = rand_filter(g, h, t, r, n_ent, big=n_ent > 30000)
    worst = 0.0
    for side, groups, anchor in ((LR.TAIL, f.tails, h), (LR.HEAD, f.heads, t)):
        qg = groups.group_of(anchor.numpy(), r.numpy())
        rk, fr, sc = K.lp_rank(ent, rel, h, t, r, norm, side, groups, qg, want_scores=True)
        true = LR.true_ids(h, t, side).to(DEV)
        mask = LR.filter_mask(groups, qg, n_ent, device=DEV)
        ar = torch.arange(B, device=DEV)
        st = sc[ar, true][:, None]
        assert torch.equal(rk, (sc >= st).sum(1))
        m = mask.clone()
        m[ar, true] = False
        assert torch.equal(fr, ((sc >= st) & ~m).sum(1))
        s64, S = LR.scores_fp64(ent, rel, h.to(DEV), t.to(DEV), r.to(DEV), norm, side)
        err = ((sc.double() - s64).abs() / S).max().item()
        worst = max(worst, err)
        assert err <= LR.TAU
        rk2, fr2 = K.lp_rank(ent, rel, h, t, r, norm, side, groups, qg)
        assert torch.equal(rk, rk2) and torch.equal(fr, fr2)
    print(f"max |err|/S = {worst:.3e}")


def one_group(ids, n_ent):
    ids = np.asarray(sorted(set(ids)), np.int64)
    return K.FilterGroups(np.array([0], np.int64), np.array([0, len(ids)], np.int64), ids, 1)


@pytest.mark.gpu
@pytest.mark.parametrize("norm", [1, 2])
def test_exact_integer_grids(gpu, norm):
    n_ent, D = 50, 8
    g = torch.Generator().manual_seed(3)
    ent = torch.randint(-3, 4, (n_ent, D), generator=g).float()
    rel = torch.randint(-2, 3, (2, D), generator=g).float()
    # tail query (h=1, r=0) with true t=5: entity 9 copies row 5 (outside the filter), entity 12 too (inside the filter)
    ent[9] = ent[5]
    ent[12] = ent[5]
    ent[20] = 0.0                                             # a zero row
    ent, rel = ent.to(DEV), rel.to(DEV)
    h, t, r = torch.tensor([1]), torch.tensor([5]), torch.tensor([0])
    s, _ = LR.scores_fp64(ent, rel, h.to(DEV), t.to(DEV), r.to(DEV), norm, LR.TAIL)
    ties_true = int((s[0] >= s[0, 5]).sum())                  # exact in fp64 and in fp32 (small integers)
    rk, fr = K.lp_rank(ent, rel, h, t, r, norm, LR.TAIL, one_group([5, 12], n_ent), [0])
    assert rk.item() == ties_true and ties_true >= 3          # the true row, 9 and 12 at least
    assert fr.item() == ties_true - 1                         # 12 filtered, 9 counts in both
    # an all-equal table: every candidate ties
    eq = torch.ones(n_ent, D, device=DEV)
    grp = [5, 7, 8, 30]
    rk, fr = K.lp_rank(eq, rel, h, t, r, norm, LR.TAIL, one_group(grp, n_ent), [0])
    assert rk.item() == n_ent and fr.item() == n_ent - len(grp) + 1
    grp = [1, 7, 8, 30]                                       # head side: the true entity is h = 1
    rk, fr = K.lp_rank(eq, rel, h, t, r, norm, LR.HEAD, one_group(grp, n_ent), [0])
    assert rk.item() == n_ent and fr.item() == n_ent - len(grp) + 1
    # n_ent = 1
    rk, fr = K.lp_rank(ent[:1].contiguous(), rel, torch.tensor([0]), torch.tensor([0]), r, norm, LR.HEAD)
    assert rk.item() == 1 and fr.item() == 1
    # zero rows everywhere: all tie
    z = torch.zeros(n_ent, D, device=DEV)
    rk, fr = K.lp_rank(z, torch.zeros(2, D, device=DEV), h, t, r, norm, LR.TAIL, one_group([5], n_ent), [0])
    assert rk.item() == n_ent and fr.item() == n_ent


@pytest.mark.gpu
def test_invariants_batch_size_repeat_and_workspace(gpu):
    g = torch.Generator().manual_seed(9)
    n_ent, D, B = 3000, 64, 700
    ent, rel = rand_tables(g, n_ent, 4, D)
    h, t, r = torch.randint(0, n_ent, (B,), generator=g), torch.randint(0, n_ent, (B,), generator=g), torch.randint(0, 4, (B,), generator=g)
    kg = K.KnowledgeGraph(h, t, r, n_ent, 4)
    f = K.KGFilters.build([kg])
    m = K.TransEPretrainModel(D, n_ent, 4).to(DEV)
    m.ent_emb.weight.data.copy_(ent)
    m.rel_emb.weight.data.copy_(rel)
    res = []
    for bs in (1, 7, B, B):
        ev = K.LinkPredictionEvaluator(m, kg, f)
        with pytest.raises(RuntimeError):
            ev.mrr()
        ev.evaluate(bs)
        res.append([ev.rank_true_heads, ev.rank_true_tails, ev.filt_rank_true_heads, ev.filt_rank_true_tails])
    for other in res[1:]:
        for a, b in zip(res[0], other):
            assert torch.equal(a, b)
    rh, rt, fh, ft = res[0]
    assert bool((fh >= 1).all() and (fh <= rh).all() and (ft >= 1).all() and (ft <= rt).all())
    # a group holding only the true id: filt_rank == rank
    only = K.FilterGroups(np.arange(B, dtype=np.int64), np.arange(B + 1, dtype=np.int64), t.numpy().copy(), 1)
    rk, fr = K.lp_rank(ent, rel, h, t, r, 2, LR.TAIL, only, np.arange(B))
    assert torch.equal(rk, fr) and torch.equal(rk.cpu(), rt)
    # one workspace reused across shapes
    ws = torch.empty(_lib.load().ia_kgpt_lp_workspace_bytes(B, D), device=DEV, dtype=torch.uint8)
    for n in (B, 5, B):
        rk, _ = K.lp_rank(ent, rel, h[:n], t[:n], r[:n], 2, LR.TAIL, workspace=ws)
        assert torch.equal(rk.cpu(), rt[:n])


@pytest.mark.gpu
def test_abi_refusals_and_out_of_range_ids(gpu):
    lib = _lib.load()
    n_ent, D, B = 100, 16, 6
    g = torch.Generator().manual_seed(1)
    ent, rel = rand_tables(g, n_ent, 3, D)
    h = torch.tensor([1, -1, 100, 2, 3, 4], device=DEV)
    t = torch.tensor([2, 3, 4, 5, 2**40, 6], device=DEV)
    r = torch.tensor([0, 0, 0, 3, 1, 2], device=DEV)
    out = torch.full((2, B + 16), -7, dtype=torch.int64, device=DEV)      # canaries on both sides of the outputs
    rank, filt = out[0, 8:8 + B], out[1, 8:8 + B]
    nbytes = lib.ia_kgpt_lp_workspace_bytes(B, D)
    ws = torch.empty(nbytes, device=DEV, dtype=torch.uint8)
    p = lambda x: x.data_ptr()  # noqa: E731

    def call(ent_p=p(ent), D_=D, n_ent_=n_ent, norm=2, side=0, B_=B, ws_bytes=nbytes, ws_p=p(ws), rank_p=p(rank), grp=(None, None, 0, None)):
        return lib.ia_kgpt_lp_rank(ent_p, p(rel), p(h), p(t), p(r), B_, D_, n_ent_, 3, norm, side, *grp, rank_p, p(filt), None, ws_p,
                                   ws_bytes, _lib.stream_ptr())
    assert call(ent_p=None) == -1
    assert call(rank_p=None) == -1
    assert call(D_=6) == -1
    assert call(norm=3) == -1
    assert call(side=2) == -1
    assert call(B_=0) == -1
    assert call(n_ent_=0) == -1
    assert call(grp=(p(rank), None, 1, None)) == -1
    assert call(ws_bytes=nbytes - 1) == -3
    assert call(ws_p=None) == -3
    torch.cuda.synchronize()
    assert bool((out == -7).all())                                         # refusals launch nothing
    for side in (0, 1):
        assert call(side=side) == 0
        torch.cuda.synchronize()
        assert out[:, 8:8 + B][:, 1:5].eq(0).all() and out[:, 8:8 + B][:, [0, 5]].ge(1).all()
        assert out[:, :8].eq(-7).all() and out[:, 8 + B:].eq(-7).all()


@pytest.mark.gpu
def test_more_query_tiles_than_one_grid_holds(gpu):
    """B = 65 535 * 128 + 5 queries: the scan's query tiles pass grid y's cap and are launched in two parts."""
    B, n_ent, D = 65535 * 128 + 5, 3, 4
    ent = torch.tensor([[0., 0., 0., 0.], [1., 0., 0., 0.], [0., 2., 0., 0.]], device=DEV)
    rel = torch.zeros(1, D, device=DEV)
    g = torch.Generator(device=DEV).manual_seed(2)
    h = torch.randint(0, n_ent, (B,), device=DEV, generator=g)
    t = torch.randint(0, n_ent, (B,), device=DEV, generator=g)
    r = torch.zeros(B, dtype=torch.int64, device=DEV)
    rk, fr = K.lp_rank(ent, rel, h, t, r, 2, LR.TAIL)
    d = ((ent[h][:, None, :] - ent[None]) ** 2).sum(-1)              # small integers: exact
    want = (d <= d.gather(1, t[:, None])).sum(1)
    assert torch.equal(rk, want) and torch.equal(fr, want)


@pytest.mark.gpu
def test_lp_rank_refuses_tables_it_would_misread(gpu):
    ent = torch.randn(10, 8, device=DEV)
    rel = torch.randn(2, 8, device=DEV)
    ids = torch.zeros(3, dtype=torch.int64)
    for bad_ent, bad_rel in ((ent.t().contiguous().t(), rel), (ent.double(), rel), (ent, rel[:, :4]), (ent, rel.cpu()),
                             (torch.randn(10, 16, device=DEV)[:, ::2], rel)):
        with pytest.raises(ValueError):
            K.lp_rank(bad_ent, bad_rel, ids, ids, ids, 2, LR.TAIL)


@pytest.mark.gpu
def test_full_size_ranks_in_the_bracket(gpu):
    import time
    n_ent, n_rel, D, B = 258211, 1379, 768, 4096
    g = torch.Generator(device=DEV).manual_seed(5)
    ent = torch.randn(n_ent, D, device=DEV, generator=g) * 0.05
    rel = torch.randn(n_rel, D, device=DEV, generator=g) * 0.05
    h = torch.randint(0, n_ent, (B,), device=DEV, generator=g)
    t = torch.randint(0, n_ent, (B,), device=DEV, generator=g)
    r = torch.randint(0, n_rel, (B,), device=DEV, generator=g)
    ent[t[:32]] = ent[h[:32]] + rel[r[:32]] + 0.01 * torch.randn(32, D, device=DEV, generator=g)   # a few well-ranked facts
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    res = {side: K.lp_rank(ent, rel, h, t, r, 2, side) for side in (LR.TAIL, LR.HEAD)}
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    print(f"full size: {B} facts, both sides, {dt * 1e3:.1f} ms")
    pick = torch.cat([torch.arange(16, device=DEV), torch.randperm(B, device=DEV, generator=g)[:48]])
    for side, (rk, fr) in res.items():
        assert torch.equal(rk, fr)
        s, S = LR.scores_fp64(ent, rel, h[pick], t[pick], r[pick], 2, side, chunk=8)
        lo, hi = LR.bracket(s, S, LR.true_ids(h[pick], t[pick], side))
        got = rk[pick]
        assert bool(((got >= lo) & (got <= hi)).all())
    assert res[LR.TAIL][0][:16].float().mean() < 100


def run_cli(*args):
    env = dict(os.environ, PYTHONNOUSERSITE="1")
    return subprocess.run([sys.executable, os.path.join(ROOT, "pkgm_pretrain.py"), *args], capture_output=True, text=True, env=env,
                          timeout=300)


def write_data(d, z):
    for s in ("train", "valid", "test"):
        with open(os.path.join(d, f"{s}2id.txt"), "w") as f:
            f.writelines(f"{h}\t{r}\t{t}\n" for h, r, t in zip(z[f"{s}_h"].tolist(), z[f"{s}_r"].tolist(), z[f"{s}_t"].tolist()))
    with open(os.path.join(d, "entity2id.txt"), "w") as f:
        f.writelines(f"/item/{i}\t{i}\n" for i in range(300))
    with open(os.path.join(d, "relation2id.txt"), "w") as f:
        f.writelines(f"rel_{i}\t{i}\n" for i in range(8))


LINE = re.compile(r"^(Hit@10 : .*|Mean Rank : .*|MRR : .*)$", re.M)


@pytest.mark.gpu
def test_cli_end_to_end(gpu, tmp_path):
    z = golden("transe_l2")
    write_data(tmp_path, z)
    common = ["--data_dir", str(tmp_path), "--model_name", "transe_epoch-{}.bin", "--num_train_epochs", "2", "--train_batch_size", "512",
              "--dim", "64", "--eval_batch_size", "33"]
    a = run_cli(*common, "--output_dir", str(tmp_path / "a"), "--do_eval", "--do_test")
    assert a.returncode == 0, a.stderr[-2000:]
    b = run_cli(*common, "--output_dir", str(tmp_path / "b"))
    assert b.returncode == 0, b.stderr[-2000:]
    ca, cb = (torch.load(tmp_path / d / "transe_epoch-2.bin") for d in ("a", "b"))
    assert sorted(ca) == sorted(cb) and all(torch.equal(ca[k], cb[k]) for k in ca)
    lines = LINE.findall(a.stdout)
    assert len(lines) == 6 and a.stdout.index("valid\n") < a.stdout.index("Hit@10")
    m = K.TransEPretrainModel(64, 300, 8)
    m.load_state_dict(ca)
    m = m.to(DEV)
    f = K.KGFilters.build([kg_of(z, s) for s in ("train", "valid", "test")])
    want = ""
    for s in ("valid", "test"):
        ev = K.LinkPredictionEvaluator(m, kg_of(z, s), f)
        ev.evaluate(1000)
        want += ev.results_text()
    assert "\n".join(lines) + "\n" == want
    # the golden tables, no training: the test-only run prints what the evaluator gives on those tables, which is torchkge's text
    path = tmp_path / "golden.bin"
    torch.save({k[3:]: torch.from_numpy(z[k]) for k in z.files if k.startswith("sd_")}, path)
    c = run_cli(*common[:4], "--num_train_epochs", "0", "--dim", "64", "--output_dir", str(tmp_path / "c"), "--pretrained_model_path",
                str(path), "--do_test")
    assert c.returncode == 0, c.stderr[-2000:]
    got = "\n".join(LINE.findall(c.stdout)) + "\n"
    ev = K.LinkPredictionEvaluator(model_of(z, "transe_l2"), kg_of(z, "test"), K.KGFilters.build([kg_of(z, s) for s in ("train", "test")]))
    ev.evaluate(1000)
    assert got == ev.results_text()
    assert got == bytes(z["t_text"]).decode()
