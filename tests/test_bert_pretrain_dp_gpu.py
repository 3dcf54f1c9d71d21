"""BertForPreTraining under data parallelism (forward(..., loss_shares=...)): two ranks, each with its dist.deal_rows slice of a
batch, must take the optimiser step of one process on the whole batch -- the masked-LM loss the mean over the labelled rows of both
slices, the next-sentence loss the mean over all rows.  The tiny configuration and the features of
tests/test_bert_pretrain_model_gpu.py, both dropouts 0.  On a one-GPU box both ranks share cuda:0 over gloo (tests/test_dp_gpu.py).

The batches are rows of those features (labelled positions per row: 3, 1, 6, 0, ...):
  * even: rows 0-3 dealt 2 + 2, with 4 and 6 labelled positions -- a plain mean of the two rank losses would be wrong;
  * two_and_one: rows 0-2 dealt 2 + 1;
  * rank_1_unlabelled: rows 0, 2, 3 dealt 2 + 1, rank 1 holds the row without a label: its masked-LM term is exactly 0, it launches
    no head kernel and still takes part in every collective.

Bars: those of tests/test_dp_gpu.py -- rtol 5e-3 on the loss and on each of its two parts, every parameter's averaged gradient within
2e-2 of that parameter's largest one-process gradient element; parameters whose gradient is numerically empty (below 1e-3 of the
largest gradient element of the model) are skipped as there, but never the four named in ALWAYS.  Every figure is printed before it is
asserted (`-s` shows them).
"""
import os
import socket
from types import SimpleNamespace

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

pytestmark = pytest.mark.gpu

CASES = {"even": (0, 1, 2, 3), "two_and_one": (0, 1, 2), "rank_1_unlabelled": (0, 2, 3)}
ALWAYS = ("bert.embeddings.word_embeddings.weight", "bert.encoder.layer.0.attention.self.query.weight",
          "cls.predictions.transform.dense.weight", "cls.seq_relationship.weight")


def _free_port():
    s = socket.socket(); s.bind(("127.0.0.1", 0)); p = s.getsockname()[1]; s.close(); return p


def _build():
    """the seeded tiny model, the same on every rank and in the one process; 1-D parameters off their 0 / 1 initial values"""
    import item_alignment_amd.models as M
    from test_bert_pretrain_model_gpu import config
    torch.manual_seed(1234)
    model = M.BertForPreTraining(SimpleNamespace(**config(hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0)))
    g = torch.Generator().manual_seed(5)
    with torch.no_grad():
        for _, p in model.named_parameters():
            if p.dim() == 1:
                p.add_(torch.randn(p.shape, generator=g) * 0.05)
    return model.cuda().train()


def _step(case, rank, world):
    """one optimiser step -> (loss, its two parts, labelled rows here, master weights after the step, the gradient the optimiser
    consumed, spans)"""
    from item_alignment_amd import dist as iadist
    from item_alignment_amd.models import functional as Fn
    from test_bert_pretrain_model_gpu import features
    model = _build()
    arena = model.param_arena
    batch = [t[list(CASES[case])] for t in features()]
    reducer, shares = None, None
    Fn.clear_grad_ready_hooks()
    if world > 1:
        lo, hi = iadist.deal_rows(len(CASES[case]), rank, world)
        batch = [t[lo:hi] for t in batch]
        iadist.broadcast_arena(arena)
        reducer = iadist.GradBucketReducer.for_arena(arena, bucket_bytes=64 << 10)     # many small buckets
        Fn.register_grad_ready_hook(reducer.grads_ready)
    ids, mask, labels, nsp = (t.cuda() for t in batch)
    n_here = int((labels != -1).sum())
    if world > 1:
        shares, totals = iadist.loss_shares([n_here, ids.shape[0]])
        assert totals[1] == len(CASES[case])
    Fn.set_step_seed(0)
    Fn.reset_use_counts()
    arena.zero_grad()
    loss = model(ids, token_type_ids=None, attention_mask=mask, masked_lm_labels=labels, next_sentence_label=nsp, loss_shares=shares)[0]
    loss.backward()
    scale = reducer.finish() if reducer is not None else 1.0
    grad = (arena.grad.detach().float() * scale).cpu().clone()
    arena.adamw_step(1e-4, grad_scale=scale)
    torch.cuda.synchronize()
    Fn.clear_grad_ready_hooks()
    spans = [(n, o, p.numel()) for n, p, o in zip(arena.names, arena.params, arena.offsets)]
    parts = [float(x) for x in model.last_losses]
    return float(loss.detach()), parts, n_here, arena.master.detach().float().cpu().clone(), grad, spans


def _worker(rank, world, port, case, out):
    os.environ.update(RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    if torch.cuda.device_count() < world:
        os.environ["IA_DP_BACKEND"] = "gloo"         # both ranks on the one GPU
    from item_alignment_amd import dist as iadist
    import importlib
    importlib.reload(iadist)                           # picks up IA_DP_BACKEND
    iadist.init_from_env("cuda")
    loss, parts, live, master, grad, _ = _step(case, rank, world)
    out[rank] = (loss, parts, live, master.numpy(), grad.numpy())
    torch.distributed.destroy_process_group()


@pytest.fixture(scope="module")
def one_process(gpu):
    """the step of one process on the whole batch, once per case; never modified"""
    return {case: _step(case, 0, 1) for case in CASES}


@pytest.mark.parametrize("case", list(CASES))
def test_two_ranks_take_the_step_of_one_process_on_the_whole_batch(gpu, one_process, case):
    world = 2
    ref_loss, ref_parts, ref_live, _, ref_grad, spans = one_process[case]
    out = mp.Manager().dict()
    mp.spawn(_worker, args=(world, _free_port(), case, out), nprocs=world, join=True)
    (l0, p0, n0, m0, g0), (l1, p1, n1, m1, g1) = out[0], out[1]
    print(f"[bert dp] {case}: labelled rows {n0} + {n1} (one process {ref_live})")
    assert np.array_equal(m0, m1) and np.array_equal(g0, g1), "replicas diverged"
    assert n0 + n1 == ref_live and n0 != n1                  # unequal shares: the plain mean of the rank losses is not the global mean
    if case == "rank_1_unlabelled":
        assert n1 == 0 and p1[0] == 0.0 and n0 > 0           # the rank without a labelled row adds exactly 0 and finishes
    else:
        assert n0 > 0 and n1 > 0
    # the mean of the weighted rank losses is the one-process loss, part by part
    for name, got, want in (("loss", (l0 + l1) / 2, ref_loss), ("masked-LM", (p0[0] + p1[0]) / 2, ref_parts[0]),
                            ("next-sentence", (p0[1] + p1[1]) / 2, ref_parts[1])):
        print(f"[bert dp] {case} {name}: {got:.6f} against {want:.6f}")
        assert abs(got - want) <= 5e-3 * abs(want), (name, got, want)
    # the averaged gradient every rank hands to the optimiser = the gradient of the whole batch, parameter by parameter
    ref_grad = ref_grad.numpy()
    gmax = np.abs(ref_grad).max()
    names = [n for n, _, _ in spans]
    always = set(ALWAYS)
    assert always <= set(names), sorted(always - set(names))
    compared, worst = set(), ("", 0.0)
    for name, off, n in spans:
        want, got = ref_grad[off:off + n], g0[off:off + n]
        if np.abs(want).max() < 1e-3 * gmax and name not in always:
            continue                                  # numerically empty gradient (untouched rows, cancelled sums)
        assert np.abs(want).max() > 0, name
        err = np.abs(got - want).max() / np.abs(want).max()
        compared.add(name)
        if name in always:
            print(f"[bert dp] {case} grad {name}: {err:.2e} of its largest element")
        worst = max(worst, (name, err), key=lambda x: x[1])
        assert err < 2e-2, (name, err)
    print(f"[bert dp] {case}: {len(compared)} of {len(names)} parameters compared, worst {worst[0]} {worst[1]:.2e}")
    assert always <= compared


def test_a_rank_without_labelled_rows_adds_zero_and_no_labelled_row_anywhere_stays_nan(gpu):
    """the two meanings of "this rank has no labelled row", in one process: weight 0 (another rank has some) makes the masked-LM term
    exactly 0, weight NaN (dist.loss_shares when no rank has one) keeps the NaN of one process; without loss_shares nothing changes"""
    from test_bert_pretrain_model_gpu import features
    model = _build()
    ids, mask, labels, nsp = (t[3:4].cuda() for t in features())          # the row without a label
    assert int((labels != -1).sum()) == 0
    with torch.no_grad():
        plain = model(ids, attention_mask=mask, masked_lm_labels=labels, next_sentence_label=nsp)[0]
        nsp_alone = float(model.last_losses[1])
        zero = model(ids, attention_mask=mask, masked_lm_labels=labels, next_sentence_label=nsp, loss_shares=(0.0, 0.5))[0]
        parts = [float(x) for x in model.last_losses]
        nan = model(ids, attention_mask=mask, masked_lm_labels=labels, next_sentence_label=nsp, loss_shares=(float("nan"), 0.5))[0]
    print(f"[bert dp] unlabelled row: plain {float(plain)}, weight 0 -> {float(zero)} = {parts}, weight NaN -> {float(nan)}")
    assert torch.isnan(plain) and torch.isnan(nan)
    assert parts[0] == 0.0 and parts[1] == 0.5 * nsp_alone and float(zero) == parts[1]
