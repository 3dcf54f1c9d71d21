"""tests/ivf_reference.py against itself, without a GPU: select_probed with every list probed is select; select_groups of one group is
select, and with labels it orders ties by the label; the CPU model of scan + fold equals select_probed bit for bit on exact operands
(whole numbers in [-4, 4]: every score is exact and full of ties), and each of its four injected faults is refused by that comparison;
check_layout accepts a stable sort of the assignment and refuses a list whose rows do not ascend."""
import numpy as np
import pytest
import torch

import ivf_reference as IR
import simtopk_reference as SR

N, D, NLIST, K = 300, 8, 7, 10


def _case():
    g = torch.Generator().manual_seed(3)
    distinct = torch.randint(-4, 5, (60, D), generator=g).to(torch.float32)
    x = distinct[torch.randint(0, 60, (N,), generator=g)]      # every row has duplicates, spread over the lists
    assignment = torch.randint(0, NLIST, (N,), generator=g).numpy()
    scores = SR.scores_fp64(x, x).astype(np.float32)
    rng = np.random.default_rng(4)
    probes = np.stack([rng.permutation(NLIST)[:3] for _ in range(N)])
    return x, assignment, scores, probes


def _same(a, b):
    return np.array_equal(a[0], b[0]) and np.array_equal(a[1].view(np.int32), b[1].view(np.int32))


def test_every_list_probed_is_the_exact_selection():
    _, assignment, scores, _ = _case()
    every = np.tile(np.arange(NLIST), (N, 1))
    skip = np.arange(N)
    assert _same(IR.select_probed(scores, assignment, every, K, skip), SR.select(scores, K, skip))
    assert _same(IR.select_probed(scores, assignment, every, 64), SR.select(scores, 64))


def test_select_groups_of_one_group_and_with_labels():
    x, _, scores, _ = _case()
    q = x[:40]
    one = IR.select_groups(q, x, [0, 40], [0, N], K, skip=np.arange(40))
    assert _same(one, SR.select(scores[:40], K, np.arange(40)))
    # the catalogue stored in reverse with label = the original row: the same lists as without the permutation
    rev = torch.arange(N - 1, -1, -1)
    got = IR.select_groups(q, x[rev], [0, 40], [0, N], K, label=rev, skip=N - 1 - np.arange(40))
    assert _same(got, one)
    # two groups, the second without queries, rows before the first offset: untouched
    two = IR.select_groups(q, x, [5, 40, 40], [0, 100, N], K)
    assert (two[0][:5] == -1).all() and np.isneginf(two[1][:5]).all()
    assert _same((two[0][5:], two[1][5:]), SR.select(scores[5:40, :100], K))


def test_the_model_of_scan_and_fold_passes():
    _, assignment, scores, probes = _case()
    skip = np.arange(N)
    for k in (1, K, 64):
        assert _same(IR.model_ivf(scores, assignment, probes, k, skip), IR.select_probed(scores, assignment, probes, k, skip)), k
        assert _same(IR.model_ivf(scores, assignment, probes, k), IR.select_probed(scores, assignment, probes, k)), k


@pytest.mark.parametrize("fault", IR.FAULTS)
def test_an_injected_fault_is_refused(fault):
    _, assignment, scores, probes = _case()
    skip = np.arange(N)
    assert not _same(IR.model_ivf(scores, assignment, probes, K, skip, fault=fault), IR.select_probed(scores, assignment, probes, K, skip)), fault


def test_lloyd_sums():
    x, assignment, _, _ = _case()
    sums, counts = IR.lloyd_sums_fp64(x, assignment, NLIST + 1)            # the last list is empty
    assert counts.sum() == N and counts[-1] == 0 and (sums[-1] == 0).all()
    assert np.array_equal(sums[2], x[torch.as_tensor(assignment == 2)].to(torch.float64).sum(0).numpy())


def test_check_layout():
    _, assignment, _, _ = _case()
    row_id = np.argsort(assignment, kind="stable")
    inv = np.empty(N, np.int64)
    inv[row_id] = np.arange(N)
    list_off = np.concatenate([[0], np.cumsum(np.bincount(assignment, minlength=NLIST))])
    IR.check_layout(row_id, inv, list_off, assignment)
    bad = row_id.copy()
    bad[[0, 1]] = bad[[1, 0]]                                              # list 0 no longer ascends
    bad_inv = np.empty(N, np.int64)
    bad_inv[bad] = np.arange(N)
    with pytest.raises(AssertionError, match="ascend"):
        IR.check_layout(bad, bad_inv, list_off, assignment)
    with pytest.raises(AssertionError):
        IR.check_layout(row_id, inv, list_off[:-1], assignment)
