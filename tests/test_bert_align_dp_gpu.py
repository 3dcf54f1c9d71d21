"""BertAlignModel under data parallelism: two ranks, each with a contiguous slice of the four pairs of
tests/test_bert_align_model_gpu.py (field lengths 40 / 24 / 8 / 16 / 8, ragged valid lengths), must take the optimiser step of one
process on the whole batch.  Each rank scales its mean cross-entropy by dist.loss_shares -- pairs here * world / pairs in all -- as
finetune_bert.py does.  The tiny configuration of that file, both dropouts 0.  On a one-GPU box both ranks share cuda:0 over gloo
(tests/test_dp_gpu.py).

Deals: 2 + 2 (dist.deal_rows' own) and 3 + 1.  Every rank's ragged pass packs a different number of valid tokens (printed), and with
3 + 1 also a different number of sequences: the point of that case -- the plain mean of the two rank losses would weigh the single
pair of rank 1 like the three of rank 0.

Bars: those of tests/test_dp_gpu.py -- rtol 5e-3 on the loss, every parameter's averaged gradient within 2e-2 of that parameter's
largest one-process gradient element; parameters whose gradient is numerically empty (below 1e-3 of the model's largest gradient
element) are skipped as there, but never the four named in ALWAYS.  Every figure is printed before it is asserted (`-s`).
"""
import os
import socket
from types import SimpleNamespace

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

pytestmark = pytest.mark.gpu

CASES = {"even": ((0, 2), (2, 4)), "three_and_one": ((0, 3), (3, 4))}
ALWAYS = ("bert.embeddings.word_embeddings.weight", "bert.encoder.layer.0.attention.self.query.weight", "bert.pooler.dense.weight",
          "cls.seq_relationship.weight")


def _free_port():
    s = socket.socket(); s.bind(("127.0.0.1", 0)); p = s.getsockname()[1]; s.close(); return p


def _build():
    """the seeded tiny model, the same on every rank and in the one process; 1-D parameters off their 0 / 1 initial values"""
    import item_alignment_amd.models as M
    from test_bert_align_model_gpu import config
    torch.manual_seed(1234)
    model = M.BertAlignModel(SimpleNamespace(**config(hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0)))
    g = torch.Generator().manual_seed(5)
    with torch.no_grad():
        for _, p in model.named_parameters():
            if p.dim() == 1:
                p.add_(torch.randn(p.shape, generator=g) * 0.05)
    return model.cuda().train()


def _step(case, rank, world):
    """one optimiser step -> (loss as it went into backward, valid tokens here, master weights after the step, the gradient the
    optimiser consumed, spans)"""
    from item_alignment_amd import dist as iadist
    from item_alignment_amd.models import functional as Fn
    from test_bert_align_model_gpu import B, features
    model = _build()
    arena = model.param_arena
    kw, labels = features()
    reducer, weight = None, 1.0
    Fn.clear_grad_ready_hooks()
    if world > 1:
        lo, hi = CASES[case][rank]
        if case == "even":
            assert (lo, hi) == iadist.deal_rows(B, rank, world)
        kw, labels = {k: v[lo:hi] for k, v in kw.items()}, labels[lo:hi]
        iadist.broadcast_arena(arena)
        reducer = iadist.GradBucketReducer.for_arena(arena, bucket_bytes=64 << 10)     # many small buckets
        Fn.register_grad_ready_hook(reducer.grads_ready)
        (weight,), (total,) = iadist.loss_shares([hi - lo])
        assert total == B and weight == (hi - lo) * world / B
    tokens = int(sum(v.sum() for k, v in kw.items() if k.endswith("attention_mask")))
    Fn.set_step_seed(0)
    Fn.reset_use_counts()
    arena.zero_grad()
    loss = model(next_sentence_label=labels.cuda(), **{k: v.cuda() for k, v in kw.items()})[-1]
    if world > 1:
        loss = loss * weight
    loss.backward()
    scale = reducer.finish() if reducer is not None else 1.0
    grad = (arena.grad.detach().float() * scale).cpu().clone()
    arena.adamw_step(1e-4, grad_scale=scale)
    torch.cuda.synchronize()
    Fn.clear_grad_ready_hooks()
    spans = [(n, o, p.numel()) for n, p, o in zip(arena.names, arena.params, arena.offsets)]
    return float(loss.detach()), tokens, arena.master.detach().float().cpu().clone(), grad, spans


def _worker(rank, world, port, case, out):
    os.environ.update(RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    if torch.cuda.device_count() < world:
        os.environ["IA_DP_BACKEND"] = "gloo"         # both ranks on the one GPU
    from item_alignment_amd import dist as iadist
    import importlib
    importlib.reload(iadist)                           # picks up IA_DP_BACKEND
    iadist.init_from_env("cuda")
    loss, tokens, master, grad, _ = _step(case, rank, world)
    out[rank] = (loss, tokens, master.numpy(), grad.numpy())
    torch.distributed.destroy_process_group()


@pytest.fixture(scope="module")
def one_process(gpu):
    """the step of one process on the four pairs; never modified"""
    return _step("even", 0, 1)


@pytest.mark.parametrize("case", list(CASES))
def test_two_ranks_take_the_step_of_one_process_on_the_whole_batch(gpu, one_process, case):
    world = 2
    ref_loss, ref_tokens, _, ref_grad, spans = one_process
    out = mp.Manager().dict()
    mp.spawn(_worker, args=(world, _free_port(), case, out), nprocs=world, join=True)
    (l0, t0, m0, g0), (l1, t1, m1, g1) = out[0], out[1]
    print(f"[bert align dp] {case}: valid tokens {t0} + {t1} (one process {ref_tokens})")
    assert np.array_equal(m0, m1) and np.array_equal(g0, g1), "replicas diverged"
    assert t0 + t1 == ref_tokens and t0 != t1 and t0 > 0 and t1 > 0          # each rank's ragged pass holds another token count
    got = (l0 + l1) / 2                                                        # the mean of the weighted rank losses
    print(f"[bert align dp] {case} loss: {got:.6f} against {ref_loss:.6f}")
    assert abs(got - ref_loss) <= 5e-3 * abs(ref_loss), (got, ref_loss)
    # the averaged gradient every rank hands to the optimiser = the gradient of the whole batch, parameter by parameter
    ref_grad = ref_grad.numpy()
    gmax = np.abs(ref_grad).max()
    names = [n for n, _, _ in spans]
    always = set(ALWAYS)
    assert always <= set(names), sorted(always - set(names))
    compared, worst = set(), ("", 0.0)
    for name, off, n in spans:
        want, have = ref_grad[off:off + n], g0[off:off + n]
        if np.abs(want).max() < 1e-3 * gmax and name not in always:
            continue                                  # numerically empty gradient (untouched rows, cancelled sums)
        assert np.abs(want).max() > 0, name
        err = np.abs(have - want).max() / np.abs(want).max()
        compared.add(name)
        if name in always:
            print(f"[bert align dp] {case} grad {name}: {err:.2e} of its largest element")
        worst = max(worst, (name, err), key=lambda x: x[1])
        assert err < 2e-2, (name, err)
    print(f"[bert align dp] {case}: {len(compared)} of {len(names)} parameters compared, worst {worst[0]} {worst[1]:.2e}")
    assert always <= compared
