"""tests/contrastive_reference.py against torch.nn.functional.cross_entropy and its autograd, both in fp64 on the CPU: the reference the
GPU test compares the kernels with has to be right first.  The shapes, scales and input kinds are those of the GPU test."""
import math

import pytest
import torch
import torch.nn.functional as F

import contrastive_reference as R

F64 = torch.float64
DLOSS = 0.75


def torch_loss(t, im, ls):
    sim = (t @ im.T) * ls.exp()
    target = torch.arange(t.shape[0])
    return 0.5 * (F.cross_entropy(sim, target) + F.cross_entropy(sim.T, target)), sim


def agree(name, got, want, rel=1e-11):
    tol = rel * max(1.0, float(want.abs().max()))
    assert float((got - want).abs().max()) <= tol, (name, float((got - want).abs().max()), tol)


@pytest.mark.parametrize("kind", R.KINDS)
@pytest.mark.parametrize("log_scale", R.LOG_SCALES)
@pytest.mark.parametrize("B,H", R.SHAPES)
def test_forward_and_backward_match_torch(B, H, log_scale, kind):
    t32, im32 = R.build(B, H, kind, seed=B + H)
    ls32 = torch.tensor(log_scale, dtype=torch.float32)
    t = t32.to(F64).requires_grad_(True)
    im = im32.to(F64).requires_grad_(True)
    ls = ls32.to(F64).requires_grad_(True)
    loss, sim = torch_loss(t, im, ls)
    (loss * DLOSS).backward()
    f = R.forward(t32, im32, float(ls32))
    agree("sim", f["sim"], sim.detach())
    agree("loss", f["loss"], loss.detach())
    agree("lse_row", f["lse_row"], torch.logsumexp(sim.detach(), 1))
    agree("lse_col", f["lse_col"], torch.logsumexp(sim.detach(), 0))
    b = R.backward(t32, im32, float(ls32), dloss=DLOSS, fwd=f)
    # the gradients cancel from terms of the size of |G| |sim|: the agreement is relative to those
    agree("dtext", b["dtext"], t.grad, rel=1e-9)
    agree("dimage", b["dimage"], im.grad, rel=1e-9)
    scale = max(1.0, float((b["G"] * f["sim"]).abs().sum()))
    assert abs(float(b["dlog_scale"]) - float(ls.grad)) <= 1e-11 * scale
    for k in ("sim_bound", "lse_row_bound", "lse_col_bound", "loss_bound"):
        assert (f[k] > 0).all() and torch.isfinite(f[k]).all(), k
    for k in ("G_bound", "dtext_bound", "dimage_bound", "dlog_scale_bound"):
        assert (b[k] > 0).all() and torch.isfinite(b[k]).all(), k


@pytest.mark.parametrize("B,H", R.SHAPES)
def test_equal_rows_give_ln_b(B, H):
    t, im = R.build(B, H, "equal", seed=3)
    f = R.forward(t, im, 1.0)
    assert abs(float(f["loss"]) - math.log(B)) <= 1e-12 * max(1.0, abs(float(f["sim"][0, 0])))


def test_batch_of_one_is_all_zero():
    t, im = R.build(1, 64, "random", seed=1)
    f = R.forward(t, im, 1.0)
    b = R.backward(t, im, 1.0, fwd=f)
    assert float(f["loss"]) == 0.0 and float(b["dlog_scale"]) == 0.0
    assert (b["G"] == 0).all() and (b["dtext"] == 0).all() and (b["dimage"] == 0).all()


def test_spike_and_huge_are_what_they_say():
    t, im = R.build(17, 192, "spike", seed=2)
    sim = R.forward(t, im, 0.0)["sim"]
    rest = sim[0].clone()
    rest[16] = -math.inf
    assert float(sim[0, 16] - rest.max()) > 40.0 and float(sim[0, 16] - sim[1:].max()) > 40.0
    t, im = R.build(64, 768, "huge", seed=2)
    sim = R.forward(t, im, 0.0)["sim"]
    assert 3e3 < float(sim.abs().mean()) < 3e4 and float(sim.min()) < -1e4 < 1e4 < float(sim.max())


def test_accumulated_value_is_added():
    t, im = R.build(3, 128, "random", seed=4)
    a = R.backward(t, im, 0.0, dloss=DLOSS)
    b = R.backward(t, im, 0.0, dloss=DLOSS, accumulated_onto=2.5)
    assert float(b["dlog_scale"]) == float(a["dlog_scale"]) + 2.5


def test_chain_lengths():
    assert R.dot_chain(768) == 194 and R.dot_chain(1) == 3 and R.dot_chain(65) == 19
    assert R.wave_chain(64) == 7 and R.wave_chain(65) == 8 and R.wave_chain(257) == 11
