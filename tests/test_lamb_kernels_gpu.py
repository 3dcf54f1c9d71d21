"""ia_lamb_flat on a hand-built arena against the fp64 reference (tests/lamb_reference.py: the definition and the derived bars): tensors of
1, 3, 63, 64, 65, 4095, 4096, 4097, 3 * 4096 + 5 and 2^20 elements at 64-element offsets, decayed + adapted and neither, one tensor
without gradient, one without weights, one frozen (in the arena, in no table), NaN in the padding of all five buffers.  Every check
reads what one module-wide fixture computed: three consecutive steps, and single steps from the initial state with clipping, with a
limit the norm stays under, with the gradients times 4 at grad_scale 1/4, and a repeat."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import lamb_reference as R

pytestmark = pytest.mark.gpu

PLAIN = R.Hyper(lr=2e-3)
CLIPPED = R.Hyper(lr=2e-3, grad_scale=0.5, max_grad_norm=1.0)
UNDER = R.Hyper(lr=2e-3, max_grad_norm=1e4)
QUARTER = R.Hyper(lr=2e-3, grad_scale=0.25)


class Device:
    """the five buffers of an R.Arena on the GPU + the tables and workspace of ia_lamb_flat"""

    def __init__(self, arena, dev):
        from item_alignment_amd import _lib
        self.lib, self.arena = _lib.load(), arena
        chunks, tensors = arena.tables()
        self.chunks, self.tensors = torch.from_numpy(chunks).to(dev), torch.from_numpy(tensors).to(dev)
        self.bytes = self.lib.ia_lamb_workspace_bytes(len(chunks), len(tensors))
        self.workspace = torch.zeros(self.bytes, dtype=torch.uint8, device=dev)
        self.dev = dev
        self.load(arena.w, arena.g, arena.m, arena.v, arena.shadow)

    def load(self, w, g, m, v, shadow):
        self.w, self.g, self.m, self.v = (torch.from_numpy(x.copy()).to(self.dev) for x in (w, g, m, v))
        self.shadow = torch.from_numpy(shadow.view(np.int16).copy()).to(self.dev).view(torch.bfloat16)

    def step(self, hp, t):
        from item_alignment_amd._lib import check, stream_ptr
        check(self.lib.ia_lamb_flat(self.w.data_ptr(), self.g.data_ptr(), self.m.data_ptr(), self.v.data_ptr(), self.shadow.data_ptr(),
                                    self.chunks.data_ptr(), self.chunks.shape[0], self.tensors.data_ptr(), self.tensors.shape[0], *hp.args(), t,
                                    hp.grad_scale, hp.max_grad_norm, self.workspace.data_ptr(), self.bytes, stream_ptr()), "ia_lamb_flat")
        torch.cuda.synchronize()
        n = self.tensors.shape[0]
        ratios = self.workspace[16:16 + 4 * n].view(torch.float32).cpu().numpy()
        return SimpleNamespace(w=self.w.cpu().numpy(), m=self.m.cpu().numpy(), v=self.v.cpu().numpy(), g=self.g.cpu().numpy(),
                               shadow=self.shadow.view(torch.int16).cpu().numpy().view(np.uint16),
                               ratios={x.name: float(r) for x, r in zip(self.arena.trainable, ratios)})


@pytest.fixture(scope="module")
def runs(gpu):
    a = R.Arena(R.arena_tensors(), seed=5)
    first = SimpleNamespace(w=a.w.copy(), g=a.g.copy(), m=a.m.copy(), v=a.v.copy(), shadow=a.shadow.copy())
    d = Device(a, gpu)
    out = SimpleNamespace(arena=a, first=first, steps=[], before=[])
    for t in (1, 2, 3):
        out.before.append(SimpleNamespace(w=d.w.cpu().numpy(), m=d.m.cpu().numpy(), v=d.v.cpu().numpy(), g=a.g.copy()))
        out.steps.append(d.step(PLAIN, t))
        a.new_grads()
        d.g = torch.from_numpy(a.g.copy()).to(gpu)

    def single(hp, g):
        d.load(first.w, g, first.m, first.v, first.shadow)
        return d.step(hp, 1)
    out.again = single(PLAIN, first.g)
    out.clipped = single(CLIPPED, first.g)
    out.under = single(UNDER, first.g)
    out.quarter = single(QUARTER, first.g * np.float32(4.0))
    return out


def same_bits(a, b):
    return a.dtype == b.dtype and np.array_equal(a.view(np.uint32 if a.dtype == np.float32 else np.uint16),
                                                 b.view(np.uint32 if b.dtype == np.float32 else np.uint16))


@pytest.mark.parametrize("t", [1, 2, 3])
def test_three_consecutive_steps_stay_inside_the_bars(runs, t):
    """m, v and w per element and r_T per tensor, each step from the state the GPU itself left"""
    a, b, got = runs.arena, runs.before[t - 1], runs.steps[t - 1]
    _, exp = R.reference_step(a.trainable, b.w, b.g, b.m, b.v, PLAIN, t)
    R.check_step(f"gpu step {t}", a.trainable, exp, got.w, got.m, got.v, got.ratios)
    if t == 1:
        assert got.ratios["zero_w.weight"] == 1.0                                       # no weights: nothing to scale by
        assert all(got.ratios[x.name] == 1.0 for x in a.trainable if not x.adapt)
        assert all(got.ratios[x.name] != 1.0 for x in a.trainable if x.adapt and not x.zero_w)


@pytest.mark.parametrize("t", [1, 2, 3])
def test_the_shadow_is_the_bf16_of_the_weights_and_nothing_outside_the_tensors_moves(runs, t):
    a, got, first = runs.arena, runs.steps[t - 1], runs.first
    for x in a.trainable:
        assert np.array_equal(got.shadow[x.sl], R.bf16_bits(got.w[x.sl])), x.name
    mask = a.padding_mask()
    for name in ("w", "m", "v", "shadow"):
        assert same_bits(getattr(got, name)[mask], getattr(first, name)[mask]), name
    assert np.isnan(got.w[mask]).sum() == np.isnan(first.w[mask]).sum() > 0
    assert not np.isnan(got.w[~mask]).any() and not np.isnan(got.m[~mask]).any() and not np.isnan(got.v[~mask]).any()


def test_a_step_that_clips_follows_the_reference(runs):
    a, f, got = runs.arena, runs.first, runs.clipped
    s, exp = R.reference_step(a.trainable, f.w, f.g, f.m, f.v, CLIPPED, 1)
    assert s < 0.1 * CLIPPED.grad_scale                   # the case does clip, hard
    R.check_step("gpu clipped", a.trainable, exp, got.w, got.m, got.v, got.ratios)
    for x in a.trainable:
        assert np.array_equal(got.shadow[x.sl], R.bf16_bits(got.w[x.sl])), x.name


def test_a_limit_above_the_norm_changes_no_bit(runs):
    for name in ("w", "m", "v", "shadow"):
        assert same_bits(getattr(runs.under, name), getattr(runs.steps[0], name)), name
    assert runs.under.ratios == runs.steps[0].ratios


def test_gradients_times_four_at_a_quarter_scale_change_no_bit(runs):
    for name in ("w", "m", "v", "shadow"):
        assert same_bits(getattr(runs.quarter, name), getattr(runs.steps[0], name)), name
    assert runs.quarter.ratios == runs.steps[0].ratios


def test_two_runs_from_the_same_state_are_bit_equal(runs):
    for name in ("w", "m", "v", "shadow"):
        assert same_bits(getattr(runs.again, name), getattr(runs.steps[0], name)), name
    assert runs.again.ratios == runs.steps[0].ratios
