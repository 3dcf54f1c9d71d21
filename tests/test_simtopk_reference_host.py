"""The references of same-item retrieval checked on the host (no GPU): select against a brute-force sort, check_topk on a CPU model of
the kernel (bf16 rows, fp32 accumulation in a permuted k order, tiles of 128 in shuffled arrival order) -- which it must accept -- and
on three injected faults, each of which it must refuse; rows_fp64 against torch's own normalize."""
import numpy as np
import pytest
import torch

import simtopk_reference as R


def _rows(seed, n, D, dup_of=None):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(n, D, generator=g)
    if dup_of:                                                 # rows drawn from a few distinct ones: ties
        x = x[torch.randint(0, dup_of, (n,), generator=g)]
    return torch.nn.functional.normalize(x, dim=1).to(torch.bfloat16)


def test_select_matches_a_brute_force_sort():
    rng = np.random.default_rng(0)
    s = rng.integers(-3, 4, (7, 23)).astype(np.float32)        # full of ties
    skip = np.array([-1, 0, 22, 5, 5, -1, 100])
    for k in (1, 4, 23, 30):
        idx, sc = R.select(s, k, skip)
        for b in range(7):
            cands = [(-s[b, c], c) for c in range(23) if c != skip[b]]
            want = sorted(cands)[:k]
            assert idx[b, :len(want)].tolist() == [c for _, c in want]
            assert sc[b, :len(want)].tolist() == [-v for v, _ in want]
            assert (idx[b, len(want):] == -1).all() and np.isneginf(sc[b, len(want):]).all()


def test_select_with_every_candidate_skipped():
    idx, sc = R.select(np.zeros((1, 1), np.float32), 3, np.array([0]))
    assert idx.tolist() == [[-1, -1, -1]] and np.isneginf(sc).all()


@pytest.fixture(scope="module")
def case():
    q, c = _rows(1, 9, 72), _rows(2, 300, 72, dup_of=25)
    skip = np.array([-1, 3, 299, 7, -1, 0, 11, 12, 13])
    return q, c, skip, R.scores_fp64(q, c), R.bar(q, c, 128)


@pytest.mark.parametrize("k", [1, 10, 64])
def test_cpu_model_passes(case, k):
    q, c, skip, s64, bars = case
    idx, sc = R.model_topk(q, c, k, skip, seed=k)
    R.check_topk(idx, sc, s64, bars, k, skip)
    idx2, sc2 = R.model_topk(q, c, k, skip, seed=k + 100)      # another k order and arrival order: the ids may differ only inside the bars
    R.check_topk(idx2, sc2, s64, bars, k, skip)


def test_cpu_model_with_few_candidates(case):
    q, c, _, s64, bars = case
    skip = np.array([0] * 9)
    R.check_topk(*R.model_topk(q, c[:5], 10, skip), s64[:, :5], bars[:, :5], 10, skip)
    R.check_topk(*R.model_topk(q, c[:1], 3, skip), s64[:, :1], bars[:, :1], 3, skip)


def test_fault_ties_to_the_highest_id_is_refused(case):
    q, c, skip, s64, bars = case
    with pytest.raises(AssertionError, match="order"):
        R.check_topk(*R.model_topk(q, c, 40, skip, ties_high=True), s64, bars, 40, skip)


def test_fault_dropped_tail_is_refused(case):
    q, c, skip, _, _ = case
    c = c.clone()
    c[299] = q[0]                                              # the last candidate of the last tile is query 0's best by far
    s64, bars = R.scores_fp64(q, c), R.bar(q, c, 128)
    skip = np.full(9, -1)
    R.check_topk(*R.model_topk(q, c, 10, skip), s64, bars, 10, skip)
    with pytest.raises(AssertionError, match="left out"):
        R.check_topk(*R.model_topk(q, c, 10, skip, drop_tail=True), s64, bars, 10, skip)


def test_fault_skipped_id_returned_is_refused(case):
    q, c, _, _, _ = case
    c = c.clone()
    c[3] = q[1]
    s64, bars = R.scores_fp64(q, c), R.bar(q, c, 128)
    skip = np.array([-1, 3, -1, -1, -1, -1, -1, -1, -1])
    R.check_topk(*R.model_topk(q, c, 10, skip), s64, bars, 10, skip)
    with pytest.raises(AssertionError, match="skipped id"):
        R.check_topk(*R.model_topk(q, c, 10, skip, return_skipped=True), s64, bars, 10, skip)


def test_wrong_score_and_missing_slot_are_refused(case):
    q, c, skip, s64, bars = case
    idx, sc = R.model_topk(q, c, 10, skip)
    bad = sc.copy()
    bad[2, 4] += 0.01
    with pytest.raises(AssertionError):
        R.check_topk(idx, bad, s64, bars, 10, skip)
    idx2, sc2 = idx.copy(), sc.copy()
    idx2[0, 9], sc2[0, 9] = -1, -np.inf
    with pytest.raises(AssertionError, match="a used slot is empty"):
        R.check_topk(idx2, sc2, s64, bars, 10, skip)


def test_rows_fp64_matches_torch_normalize():
    g = torch.Generator().manual_seed(3)
    x = torch.randn(6, 19, generator=g)
    x[2] = 0
    want = torch.nn.functional.normalize(x.double(), dim=1, eps=1e-12)
    assert torch.equal(R.rows_fp64(x, True), want)
    assert torch.equal(R.rows_fp64(x, False), x.double())
    assert (R.rows_fp64(x, True)[2] == 0).all()
