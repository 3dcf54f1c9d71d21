"""The streaming top-k kernel (ia_kgpt_topk through kg_topk): exact against the project's own score matrix (ia_kgpt_lp_rank's stored
scores, the fp32 restatement for the relation mode) selected with numpy lexsort, ties, the filter, invalid ids, the fp64 bound of
tests/linkpred_reference.py and determinism."""
import os
import sys

import numpy as np
import pytest
import torch

from item_alignment_amd.models import kg_pretrain as K

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import kgtopk_reference as KR  # noqa: E402
import linkpred_reference as LR  # noqa: E402

DEV = "cuda"
pytestmark = pytest.mark.gpu
SPLITS = (1, 2, 7, 0)


def tables(g, n_ent, n_rel, D):
    ent = torch.randn(n_ent, D, generator=g) * (torch.rand(n_ent, 1, generator=g) * 1.5 + 0.5)
    rel = torch.randn(n_rel, D, generator=g) * 0.3
    return ent.to(DEV), rel.to(DEV)


def random_groups(g, B, n_cand, max_size=40):
    """(FilterGroups, q_grp, mask): every second query gets a group of random member ids, the others none (-1)."""
    offs, ids, q_grp = [0], [], []
    mask = np.zeros((B, n_cand), bool)
    for i in range(B):
        if i % 2:
            q_grp.append(-1)
            continue
        m = np.sort(torch.randperm(n_cand, generator=g)[:int(torch.randint(1, min(n_cand, max_size) + 1, (1,), generator=g))].numpy())
        q_grp.append(len(offs) - 1)
        ids.append(m)
        offs.append(offs[-1] + len(m))
        mask[i, m] = True
    n = len(offs) - 1
    fg = K.FilterGroups(np.arange(n, dtype=np.int64), np.asarray(offs, np.int64), np.concatenate(ids).astype(np.int64), 1)
    return fg, np.asarray(q_grp, np.int64), mask


def matrix(ent, rel, a, b, norm, mode):
    """The fp32 [B, n_cand] scores as numpy: the rank kernel's stored matrix (entity modes), the numpy restatement (relations)."""
    if mode == KR.RELS:
        return KR.relation_scores_fp32(ent, rel, a, b, norm)
    side = LR.TAIL if mode == KR.TAILS else LR.HEAD
    return K.lp_rank(ent, rel, a, a, b, norm, side, want_scores=True)[2].cpu().numpy()


def check_exact(ent, rel, a, b, norm, mode, ks, fg=None, q_grp=None, mask=None, splits=SPLITS):
    sc = matrix(ent, rel, a, b, norm, mode)
    for k in ks:
        want_i, want_s = KR.select(sc, k, mask)
        for ms in splits:
            idx, score = K.kg_topk(ent, rel, a, b, norm, mode, k, fg, q_grp, max_splits=ms)
            assert idx.dtype == torch.int64 and score.dtype == torch.float32 and idx.shape == (len(a), k)
            assert torch.equal(idx.cpu(), want_i), (k, ms)
            assert torch.equal(score.cpu(), want_s), (k, ms)                       # bit-equal (-inf == -inf)


@pytest.mark.parametrize("norm", [1, 2])
@pytest.mark.parametrize("D", [4, 20, 64])
@pytest.mark.parametrize("n_ent", [5, 129, 257, 1000])
def test_entity_modes_equal_the_matrix_path(gpu, n_ent, D, norm):
    g = torch.Generator().manual_seed(n_ent * 131 + D * 7 + norm)
    ent, rel = tables(g, n_ent, 6, D)
    B = 130
    a, b = torch.randint(0, n_ent, (B,), generator=g), torch.randint(0, 6, (B,), generator=g)
    fg, q_grp, mask = random_groups(g, B, n_ent)
    for mode in (KR.TAILS, KR.HEADS):
        check_exact(ent, rel, a, b, norm, mode, (1, 10, 64), fg, q_grp, mask)
        check_exact(ent, rel, a[:1], b[:1], norm, mode, (1, 10, 64), fg, q_grp[:1], mask[:1])         # B = 1
    check_exact(ent, rel, a, b, norm, KR.TAILS, (10,))                                                  # grp_off == NULL


@pytest.mark.parametrize("norm", [1, 2])
def test_a_split_that_walks_many_tiles(gpu, norm):
    """300 000 entities: 2 344 candidate tiles, more than the scan's target workgroup count."""
    g = torch.Generator().manual_seed(17 + norm)
    n_ent, D, B = 300000, 4, 3
    ent, rel = tables(g, n_ent, 2, D)
    a, b = torch.randint(0, n_ent, (B,), generator=g), torch.randint(0, 2, (B,), generator=g)
    fg, q_grp, mask = random_groups(g, B, n_ent)
    check_exact(ent, rel, a, b, norm, KR.TAILS, (10, 64), fg, q_grp, mask)


@pytest.mark.parametrize("norm", [1, 2])
@pytest.mark.parametrize("D", [4, 20, 64])
@pytest.mark.parametrize("n_rel", [3, 200])
def test_relation_mode_equals_the_fp32_restatement(gpu, n_rel, D, norm):
    g = torch.Generator().manual_seed(n_rel * 31 + D + norm)
    ent, rel = tables(g, 300, n_rel, D)
    B = 130
    a, b = torch.randint(0, 300, (B,), generator=g), torch.randint(0, 300, (B,), generator=g)
    fg, q_grp, mask = random_groups(g, B, n_rel)
    check_exact(ent, rel, a, b, norm, KR.RELS, (1, 10, 64), fg, q_grp, mask)
    check_exact(ent, rel, a[:1], b[:1], norm, KR.RELS, (10,), fg, q_grp[:1], mask[:1])


@pytest.mark.parametrize("norm", [1, 2])
def test_ties_come_out_lowest_id_first(gpu, norm):
    """1000 entities drawn from 40 distinct rows: exact duplicates inside a tile, across tiles and splits, and across the k-th place."""
    g = torch.Generator().manual_seed(5)
    n_ent, D, B = 1000, 20, 130
    base = torch.randn(40, D, generator=g)
    ent = base[torch.randint(0, 40, (n_ent,), generator=g)].contiguous().to(DEV)
    rel = (torch.randn(4, D, generator=g) * 0.3).to(DEV)
    a, b = torch.randint(0, n_ent, (B,), generator=g), torch.randint(0, 4, (B,), generator=g)
    fg, q_grp, mask = random_groups(g, B, n_ent)
    for mode in (KR.TAILS, KR.HEADS):
        check_exact(ent, rel, a, b, norm, mode, (1, 10, 64), fg, q_grp, mask)
    idx, score = K.kg_topk(ent, rel, a, b, norm, KR.TAILS, 64)
    same = score[:, 1:] == score[:, :-1]
    assert bool(same.any(1).all())                                                  # every query has ties among its 64
    assert bool((idx[:, 1:] > idx[:, :-1])[same].all())
    assert bool((score[:, 1:] <= score[:, :-1]).all())


def one_group(ids):
    ids = np.asarray(sorted(set(int(i) for i in ids)), np.int64)
    return K.FilterGroups(np.array([0], np.int64), np.array([0, len(ids)], np.int64), ids, 1)


@pytest.mark.parametrize("mode", [KR.TAILS, KR.HEADS])
def test_filter(gpu, mode):
    g = torch.Generator().manual_seed(23)
    n_ent, D = 1000, 20
    ent, rel = tables(g, n_ent, 3, D)
    a, b = torch.tensor([7, 7]), torch.tensor([1, 1])
    free, _ = K.kg_topk(ent, rel, a, b, 2, mode, 10)
    assert torch.equal(free[0], free[1])
    top5 = free[0, :5].tolist()
    # the unfiltered top 5 in the group of query 0; query 1 has no group (q_grp = -1)
    idx, score = K.kg_topk(ent, rel, a, b, 2, mode, 10, one_group(top5), [0, -1])
    assert not set(idx[0].tolist()) & set(top5)
    assert idx[0, :5].tolist() == free[0, 5:].tolist()
    assert torch.equal(idx[1], free[0])
    mask = np.zeros((2, n_ent), bool)
    mask[0, top5] = True
    check_exact(ent, rel, a, b, 2, mode, (10,), one_group(top5), np.array([0, -1]), mask)
    # a group that leaves 3 candidates: 3 entries, then -1 / -inf
    left = [4, 500, 999]
    members = [i for i in range(n_ent) if i not in left]
    idx, score = K.kg_topk(ent, rel, a, b, 2, mode, 10, one_group(members), [0, 5])       # 5: outside [0, n_grp) = no filter
    assert sorted(idx[0, :3].tolist()) == left and idx[0, 3:].eq(-1).all() and torch.isinf(score[0, 3:]).all() and (score[0, 3:] < 0).all()
    assert torch.isfinite(score[0, :3]).all() and torch.equal(idx[1], free[0])
    mask = np.zeros((2, n_ent), bool)
    mask[0, members] = True
    check_exact(ent, rel, a, b, 2, mode, (10,), one_group(members), np.array([0, 5]), mask)
    # 900 of 1000 ids (the binary search)
    members = torch.randperm(n_ent, generator=g)[:900].tolist()
    mask = np.zeros((2, n_ent), bool)
    mask[:, members] = True
    check_exact(ent, rel, a, b, 1, mode, (10, 64), one_group(members), np.array([0, 0]), mask)


def test_more_slots_than_candidates(gpu):
    g = torch.Generator().manual_seed(2)
    ent, rel = tables(g, 5, 3, 8)
    idx, score = K.kg_topk(ent, rel, torch.tensor([0, 4]), torch.tensor([2, 0]), 2, KR.TAILS, 10)
    assert sorted(idx[0, :5].tolist()) == [0, 1, 2, 3, 4] and idx[:, 5:].eq(-1).all() and (score[:, 5:] == -float("inf")).all()
    idx, score = K.kg_topk(ent, rel, torch.tensor([0, 4]), torch.tensor([2, 0]), 2, KR.RELS, 10)
    assert sorted(idx[1, :3].tolist()) == [0, 1, 2] and idx[:, 3:].eq(-1).all() and (score[:, 3:] == -float("inf")).all()


@pytest.mark.parametrize("mode", [KR.TAILS, KR.HEADS, KR.RELS])
def test_invalid_ids_give_an_empty_row(gpu, mode):
    g = torch.Generator().manual_seed(3)
    n_ent, n_rel = 300, 12
    ent, rel = tables(g, n_ent, n_rel, 16)
    nb = n_ent if mode == KR.RELS else n_rel
    a = torch.tensor([1, -1, n_ent, 2, 3, 4])
    b = torch.tensor([0, 0, 0, nb, -5, 2])
    idx, score = K.kg_topk(ent, rel, a, b, 2, mode, 10)
    assert idx[1:5].eq(-1).all() and (score[1:5] == -float("inf")).all()
    good = torch.tensor([0, 5])
    i2, s2 = K.kg_topk(ent, rel, a[good], b[good], 2, mode, 10)
    assert torch.equal(idx[good], i2) and torch.equal(score[good], s2) and i2.ge(0).all()


@pytest.mark.parametrize("norm", [1, 2])
@pytest.mark.parametrize("mode", [KR.TAILS, KR.HEADS, KR.RELS])
def test_fp64_bound(gpu, mode, norm):
    """Every returned score within tau S of the fp64 score of that id; every candidate neither returned nor filtered scores at most
    the k-th returned one + tau (S_c + S_kth) in fp64."""
    g = torch.Generator().manual_seed(41 + mode + norm)
    n_ent, n_rel, D, B, k = 1000, 200, 64, 130, 10
    ent, rel = tables(g, n_ent, n_rel, D)
    nb, n_cand = (n_ent, n_rel) if mode == KR.RELS else (n_rel, n_ent)
    a, b = torch.randint(0, n_ent, (B,), generator=g), torch.randint(0, nb, (B,), generator=g)
    fg, q_grp, mask = random_groups(g, B, n_cand)
    idx, score = K.kg_topk(ent, rel, a, b, norm, mode, k, fg, q_grp)
    s, S = KR.scores_fp64(ent, rel, a.to(DEV), b.to(DEV), norm, mode)
    assert idx.ge(0).all()
    s_ret, S_ret = s.gather(1, idx), S.gather(1, idx)
    err = ((score.double() - s_ret).abs() / S_ret).max().item()
    print(f"max |err|/S = {err:.3e}")
    assert err <= KR.TAU
    out = torch.from_numpy(mask).to(DEV)
    out.scatter_(1, idx, True)
    bound = s_ret[:, -1:] + KR.TAU * (S + S_ret[:, -1:])
    assert bool(((s <= bound) | out).all())


def test_determinism_and_position_independence(gpu):
    g = torch.Generator().manual_seed(8)
    n_ent, D, B = 1000, 64, 130
    ent, rel = tables(g, n_ent, 5, D)
    a, b = torch.randint(0, n_ent, (B,), generator=g), torch.randint(0, 5, (B,), generator=g)
    fg, q_grp, _ = random_groups(g, B, n_ent)
    r1 = K.kg_topk(ent, rel, a, b, 2, KR.TAILS, 10, fg, q_grp)
    r2 = K.kg_topk(ent, rel, a, b, 2, KR.TAILS, 10, fg, q_grp)
    assert torch.equal(r1[0], r2[0]) and torch.equal(r1[1], r2[1])
    alone = K.kg_topk(ent, rel, a[129:], b[129:], 2, KR.TAILS, 10, fg, q_grp[129:])
    assert torch.equal(alone[0][0], r1[0][129]) and torch.equal(alone[1][0], r1[1][129])
    # one workspace reused across shapes
    from item_alignment_amd import _lib
    ws = torch.empty(_lib.load().ia_kgpt_topk_workspace_bytes(B, D, n_ent, 10, 0), device=DEV, dtype=torch.uint8)
    for n in (B, 5, B):
        got = K.kg_topk(ent, rel, a[:n], b[:n], 2, KR.TAILS, 10, fg, q_grp[:n], workspace=ws)
        assert torch.equal(got[0], r1[0][:n]) and torch.equal(got[1], r1[1][:n])


def test_refusals_launch_nothing(gpu):
    from item_alignment_amd import _lib
    lib = _lib.load()
    g = torch.Generator().manual_seed(1)
    n_ent, D, B, k = 100, 16, 6, 4
    ent, rel = tables(g, n_ent, 3, D)
    a = torch.zeros(B, dtype=torch.int64, device=DEV)
    out_i = torch.full((B + 16, k), -7, dtype=torch.int64, device=DEV)           # canaries around the outputs
    out_s = torch.full((B + 16, k), -7.0, device=DEV)
    idx, score = out_i[8:8 + B], out_s[8:8 + B]
    nbytes = lib.ia_kgpt_topk_workspace_bytes(B, D, n_ent, k, 0)
    ws = torch.empty(nbytes, device=DEV, dtype=torch.uint8)
    p = lambda x: x.data_ptr()  # noqa: E731

    def call(ent_p=p(ent), D_=D, norm=2, mode=0, B_=B, k_=k, ms=0, ws_bytes=nbytes, ws_p=p(ws), idx_p=p(idx), grp=(None, None, 0, None)):
        return lib.ia_kgpt_topk(ent_p, p(rel), p(a), p(a), B_, D_, n_ent, 3, norm, mode, *grp, k_, ms, idx_p, p(score), ws_p, ws_bytes,
                                _lib.stream_ptr())
    assert call(ent_p=None) == -1 and call(idx_p=None) == -1 and call(D_=6) == -1 and call(norm=3) == -1 and call(mode=3) == -1
    assert call(B_=0) == -1 and call(k_=0) == -1 and call(k_=65) == -1 and call(ms=-1) == -1
    assert call(grp=(p(a), None, 1, None)) == -1
    assert call(ws_bytes=nbytes - 1) == -3 and call(ws_p=None) == -3
    torch.cuda.synchronize()
    assert bool((out_i == -7).all() and (out_s == -7).all())
    assert call() == 0
    torch.cuda.synchronize()
    assert idx.ge(0).all() and out_i[:8].eq(-7).all() and out_i[8 + B:].eq(-7).all() and out_s[:8].eq(-7).all() and out_s[8 + B:].eq(-7).all()
