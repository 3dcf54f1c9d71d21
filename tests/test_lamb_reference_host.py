"""The LAMB reference (tests/lamb_reference.py) against closed forms, an fp32 model of the kernels against the reference's bars at the
shapes of the GPU test, three deliberate mistakes that the bars must catch, and the argument checks of the two C entry points (which
return before any launch: no GPU here)."""
import numpy as np
import pytest

import lamb_reference as R


def small_arena(seed=3):
    return R.Arena([R.Tensor("x.weight", 300, True), R.Tensor("x.bias", 40, False), R.Tensor("z.weight", 70, True, zero_w=True)], seed)


def test_a_tensor_that_is_neither_decayed_nor_adapted_takes_the_bias_corrected_adam_step():
    a = small_arena()
    rng = np.random.default_rng(1)
    t = a.tensors[1]
    a.m[t.sl], a.v[t.sl] = rng.normal(0, 0.01, t.n), rng.uniform(1e-5, 1e-3, t.n)
    hp = R.Hyper(lr=1e-3, b1=0.9, b2=0.98, eps=1e-8, wd=0.0)
    _, exp = R.reference_step(a.trainable, a.w, a.g, a.m, a.v, hp, 5)
    g, m0, v0, w0 = (x[t.sl].astype(np.float64) for x in (a.g, a.m, a.v, a.w))
    m = hp.b1 * m0 + (1 - hp.b1) * g
    v = hp.b2 * v0 + (1 - hp.b2) * g * g
    adam = w0 - hp.lr * (m / (1 - hp.b1 ** 5)) / (np.sqrt(v / (1 - hp.b2 ** 5)) + hp.eps)
    e = exp[t.name]
    assert e.r == 1.0 and e.dr == 0.0
    np.testing.assert_allclose(e.w, adam, rtol=1e-14, atol=0)


def test_the_trust_ratio_does_not_depend_on_the_scale_of_the_gradients_as_eps_goes_to_zero():
    a = small_arena()
    hp = R.Hyper(lr=1e-3, eps=1e-30, wd=0.0)           # not 0: an element without gradient is 0 / (0 + eps)
    _, one = R.reference_step(a.trainable, a.w, a.g, a.m, a.v, hp, 1)
    _, big = R.reference_step(a.trainable, a.w, a.g * np.float32(1024.0), a.m, a.v, hp, 1)
    assert one["x.weight"].r == pytest.approx(big["x.weight"].r, rel=1e-13)
    # at step 1 with zero moments u = sign(g): |u| = sqrt(number of non-zero gradients)
    t = a.tensors[0]
    want = np.sqrt(np.sum(a.w[t.sl].astype(np.float64) ** 2)) / np.sqrt(np.count_nonzero(a.g[t.sl]))
    assert one["x.weight"].r == pytest.approx(want, rel=1e-13)


def test_all_zero_weights_give_ratio_one_and_clipping_follows_the_formula():
    a = small_arena()
    hp = R.Hyper(lr=1e-3, grad_scale=0.5, max_grad_norm=0.25)
    s, exp = R.reference_step(a.trainable, a.w, a.g, a.m, a.v, hp, 1)
    assert exp["z.weight"].r == 1.0 and exp["z.weight"].dr == 0.0
    norm = np.sqrt(sum(np.sum(a.g[t.sl].astype(np.float64) ** 2) for t in a.trainable))
    assert 0.5 * norm > 0.25 and s == pytest.approx(0.5 * 0.25 / (0.5 * norm + 1e-6), rel=1e-15)
    assert R.grad_factor([a.g[t.sl] for t in a.trainable], 0.5, 1e6) == 0.5
    assert R.grad_factor([a.g[t.sl] for t in a.trainable], 0.5, 0.0) == 0.5


def test_bf16_bits_round_to_nearest_even():
    x = np.asarray([1.0, 1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8, 1.0 + 2.0 ** -8 + 2.0 ** -20, -0.3], np.float32)
    import torch
    want = torch.from_numpy(x).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)
    assert (R.bf16_bits(x) == want).all()
    assert R.bf16_bits(x)[1] == 0x3F80 and R.bf16_bits(x)[2] == 0x3F82          # ties go to the even mantissa


@pytest.fixture(scope="module")
def arena():
    """the GPU test's arena with a 2^16-element tensor in place of the 2^20 one (the host model is numpy): 16 chunks, still many"""
    return R.Arena(R.arena_tensors(big=1 << 16), seed=11)


HP = dict(plain=R.Hyper(lr=2e-3), clipped=R.Hyper(lr=2e-3, grad_scale=0.5, max_grad_norm=1.0))


@pytest.mark.parametrize("which", ["plain", "clipped"])
def test_the_fp32_model_of_the_kernels_stays_inside_the_bars_for_three_steps(which):
    a = R.Arena(R.arena_tensors(big=1 << 16), seed=11)
    hp, tensors = HP[which], a.trainable
    w, m, v = a.w, a.m, a.v
    for t in (1, 2, 3):
        _, exp = R.reference_step(tensors, w, a.g, m, v, hp, t)
        w2, m2, v2, shadow, ratios = R.kernel_model_step(tensors, w, a.g, m, v, hp, t)
        top = R.check_step(f"host model {which} step {t}", tensors, exp, w2, m2, v2, ratios)
        assert top["w"] > 0.0                       # the bars were compared with something that is not the reference itself
        mask = a.padding_mask()
        assert np.isnan(w2[mask & np.isnan(w)]).all() and (w2[mask & ~np.isnan(w)] == w[mask & ~np.isnan(w)]).all()
        w, m, v = w2, m2, v2
        a.new_grads()


@pytest.mark.parametrize("fault", ["ratio_per_chunk", "padding_in_norm", "no_bias_correction"])
def test_a_wrong_kernel_falls_outside_the_bars(arena, fault):
    hp, tensors = HP["plain"], arena.trainable
    _, exp = R.reference_step(tensors, arena.w, arena.g, arena.m, arena.v, hp, 2)
    w2, m2, v2, _, ratios = R.kernel_model_step(tensors, arena.w, arena.g, arena.m, arena.v, hp, 2, fault=fault)
    with pytest.raises(AssertionError):
        R.check_step(fault, tensors, exp, w2, m2, v2, ratios)


def test_the_c_entry_points_check_their_arguments_before_any_launch():
    from item_alignment_amd import _lib
    lib = _lib.load()
    assert lib.ia_lamb_workspace_bytes(0, 3) == 0 and lib.ia_lamb_workspace_bytes(3, 0) == 0
    need = lib.ia_lamb_workspace_bytes(10, 3)
    assert need >= 16 + 4 * 3 + 3 * 4 * 10 and lib.ia_lamb_workspace_bytes(11, 3) > need
    p = 4096                      # never dereferenced: every call below is refused first
    ok = dict(params=p, grads=p, m=p, v=p, shadow=p, chunks=p, n_chunks=10, tensors=p, n_tensors=3, lr=1e-3, b1=0.9, b2=0.999, eps=1e-6,
              wd=0.01, step=1, grad_scale=1.0, max_grad_norm=0.0, workspace=p, workspace_bytes=need, stream=None)

    def call(**change):
        return lib.ia_lamb_flat(*{**ok, **change}.values())
    for name in ("params", "grads", "m", "v", "chunks", "tensors"):
        assert call(**{name: None}) == -1, name
    assert call(step=0) == -1 and call(step=-3) == -1
    assert call(n_tensors=0) == -1 and call(n_chunks=0) == -1
    assert call(workspace=None) == -3 and call(workspace_bytes=need - 1) == -3 and call(workspace_bytes=0) == -3
