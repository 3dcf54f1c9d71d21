"""tests/vocab_ce_reference.py against torch.nn.functional.cross_entropy(..., ignore_index=-1) and its autograd, both in fp64 on the
CPU: the reference the GPU test compares the kernels with has to be right first."""
import math

import pytest
import torch
import torch.nn.functional as F

import vocab_ce_reference as R

F64 = torch.float64


def case(M, V, ld, seed, ignore=()):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn((M, ld), generator=g, dtype=F64) * 3.0
    y = torch.randint(0, V, (M,), generator=g)
    for r in ignore:
        y[r] = -1
    return x, y


@pytest.mark.parametrize("M,V,ld,ignore", [(5, 1003, 1004, (1, 3)), (1, 8, 8, ()), (7, 50, 52, (0,)), (257, 100, 100, tuple(range(0, 257, 3)))])
def test_forward_and_backward_match_torch(M, V, ld, ignore):
    x, y = case(M, V, ld, 11 + M, ignore)
    ldg = (V + 7) & ~7
    xt = x[:, :V].clone().requires_grad_(True)
    loss = F.cross_entropy(xt, y, ignore_index=-1)
    (loss * 0.75).backward()
    f = R.forward(x, y, V)
    assert f["n_live"] == M - len(ignore)
    assert abs(float(f["mean"]) - loss.item()) <= 1e-12 * max(1.0, abs(loss.item()))
    per = F.cross_entropy(x[:, :V], y, ignore_index=-1, reduction="none")
    assert torch.allclose(f["loss_row"], per, rtol=0, atol=1e-12)
    live = y >= 0
    assert torch.allclose(f["lse"][live], torch.logsumexp(x[live, :V], dim=1), rtol=0, atol=1e-12)
    assert (f["lse"][~live] == 0).all() and (f["loss_row"][~live] == 0).all()
    g, bound = R.backward(x, y, V, ldg, dloss=0.75, fwd=f)
    assert torch.allclose(g[:, :V], xt.grad, rtol=0, atol=1e-14)
    assert (g[:, V:] == 0).all() and (bound[:, V:] == 0).all()
    assert (g[~live] == 0).all() and (bound[~live] == 0).all()
    assert (bound[live, :V] > 0).all() and (f["lse_bound"][live] > 0).all()


def test_pad_columns_are_not_read():
    x, y = case(4, 10, 12, 3)
    want = R.forward(x, y, 10)
    x[:, 10:] = float("nan")
    got = R.forward(x, y, 10)
    assert torch.equal(want["loss_row"], got["loss_row"]) and torch.equal(want["mean"], got["mean"])


def test_all_rows_ignored_is_nan_with_zero_gradient():
    x, _ = case(3, 16, 16, 5)
    y = torch.full((3,), -1)
    f = R.forward(x, y, 16)
    assert math.isnan(float(f["mean"])) and f["n_live"] == 0
    assert math.isnan(float(F.cross_entropy(x, y, ignore_index=-1)))
    g, b = R.backward(x, y, 16, 16, fwd=f)
    assert (g == 0).all() and (b == 0).all()


def test_label_outside_the_vocabulary():
    x, y = case(4, 16, 16, 7)
    y[2] = 16
    f = R.forward(x, y, 16)
    assert math.isnan(float(f["loss_row"][2])) and math.isnan(float(f["mean"])) and f["n_live"] == 4
    g, b = R.backward(x, y, 16, 16, fwd=f)
    assert (g[2] == 0).all() and (b[2] == 0).all() and (g[0] != 0).any()


def test_large_magnitudes_do_not_overflow():
    x = torch.full((2, 16), -1e4, dtype=F64)
    x[0, 3] = 1e4
    x[1, :] = 1e4
    y = torch.tensor([3, 0])
    f = R.forward(x, y, 16)
    assert float(f["loss_row"][0]) == 0.0
    assert abs(float(f["lse"][1]) - (1e4 + math.log(16))) < 1e-9


def test_chain_lengths():
    assert R.row_chain(21128) == 21 + 12 and R.row_chain(8) == 1 + 12
    assert R.mean_chain(3) == 21 and R.mean_chain(64 * 1024 + 1) == 22
