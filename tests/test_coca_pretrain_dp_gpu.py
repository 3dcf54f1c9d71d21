"""CoCaForPretraining under data parallelism (set_data_parallel): two ranks, each with a shard of the four-item batch of
tests/golden/coca/pretrain.npz, must take the optimiser step of one process on the whole batch -- every other item of the global batch
a contrastive negative, the caption loss the mean over the live label rows of both shards.  The tiny model of
tests/test_coca_pretrain_model_gpu.py, dropout 0.  On a one-GPU box both ranks share cuda:0 over gloo (tests/test_dp_gpu.py).

Bars: those of tests/test_dp_gpu.py -- 2e-2 of a parameter's largest gradient, rtol 5e-3 on the loss.  The one-process model computes
the same function through other kernels' summation orders (square contrastive kernels, one caption head over all live rows, GEMMs over
4 n rows instead of 2 n or 3 n / n), in bf16 activations; no parameter needed a wider bar: on an MI355X the worst parameter of the
three cases was off by 2.6e-7 of its largest element and the losses agreed to the six printed decimals (the figures are printed, `-s`).
Parameters whose gradient is numerically empty are skipped as there, but never `temperature`, the word table, `to_logits.0.gamma` or the
multimodal, text-tower and ViT weights named in ALWAYS: those are always compared.
"""
import os
import socket

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

pytestmark = pytest.mark.gpu

N = 5
# name -> (row ranges of the two shards, the label rows made pad beforehand)
CASES = {"even": ((0, 2), (2, 4), ()), "three_and_one": ((0, 3), (3, 4), ()), "one_rank_all_pad": ((0, 3), (3, 4), (3,))}
ALWAYS = ("temperature", "coca.text_encoder.embeddings.word_embeddings.weight", "to_logits.0.gamma",
          "multimodal_layers.0.0.fn.fused_attn_ff_proj.weight", "coca.text_encoder.encoder.layer.0.attention.self.query.weight",
          "coca.img_encoder.blocks.0.attn.qkv.weight")


def _free_port():
    s = socket.socket(); s.bind(("127.0.0.1", 0)); p = s.getsockname()[1]; s.close(); return p


def _golden():
    from test_coca_pretrain_model_gpu import GOLDEN
    z = np.load(GOLDEN)
    return {k: z[k] for k in z.files}


def _batch(golden, case):
    from test_coca_pretrain_model_gpu import batch
    t = batch(golden, N)
    labels = t["labels"].clone()
    for row in CASES[case][2]:
        labels[row] = 0
    t["labels"] = labels
    return t


def _step(case, rank, world):
    """one optimiser step -> (loss, the two parts, live rows, master weights after the step, the gradient the optimiser consumed, spans)"""
    from item_alignment_amd import dist as iadist
    from item_alignment_amd.models import functional as Fn
    from test_coca_pretrain_model_gpu import build, run
    golden = _golden()
    model = build(golden).train()
    arena = model.param_arena
    t = _batch(golden, case)
    reducer = None
    Fn.clear_grad_ready_hooks()
    if world > 1:
        lo, hi = CASES[case][rank]
        t = {k: v[lo:hi].contiguous() for k, v in t.items()}
        iadist.broadcast_arena(arena)
        reducer = iadist.GradBucketReducer.for_arena(arena, bucket_bytes=64 << 10)     # many small buckets
        Fn.register_grad_ready_hook(reducer.grads_ready)
        model.set_data_parallel()
    Fn.set_step_seed(0)
    Fn.reset_use_counts()
    arena.zero_grad()
    loss = run(model, t)
    loss.backward()
    scale = reducer.finish() if reducer is not None else 1.0
    grad = (arena.grad.detach().float() * scale).cpu().clone()
    arena.adamw_step(1e-4, grad_scale=scale)
    torch.cuda.synchronize()
    Fn.clear_grad_ready_hooks()
    spans = [(n, o, p.numel()) for n, p, o in zip(arena.names, arena.params, arena.offsets)]
    parts = [float(x) for x in model.last_losses]
    return float(loss.detach()), parts, model.caption_live_rows, arena.master.detach().float().cpu().clone(), grad, spans


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
    """the step of one process on the whole batch, once per label variant"""
    return {pads: _step(case, 0, 1) for case, pads in (("even", ()), ("one_rank_all_pad", (3,)))}


@pytest.mark.parametrize("case", list(CASES))
def test_two_ranks_take_the_step_of_one_process_on_the_whole_batch(gpu, one_process, case):
    world = 2
    ref_loss, ref_parts, ref_live, _, ref_grad, spans = one_process[CASES[case][2]]
    out = mp.Manager().dict()
    mp.spawn(_worker, args=(world, _free_port(), case, out), nprocs=world, join=True)
    (l0, p0, n0, m0, g0), (l1, p1, n1, m1, g1) = out[0], out[1]
    assert np.array_equal(m0, m1) and np.array_equal(g0, g1), "replicas diverged"
    assert n0 + n1 == ref_live
    if case == "three_and_one":
        assert n0 != 3 * n1 and n0 > 0 and n1 > 0            # the per-rank caption means do not average to the global mean
    if case == "one_rank_all_pad":
        assert n1 == 0 and p1[0] == 0.0 and n0 > 0           # the rank without a live row adds 0 and finishes
    # the mean of the rank losses is the one-process loss, part by part
    for name, got, want in (("loss", (l0 + l1) / 2, ref_loss), ("caption", (p0[0] + p1[0]) / 2, ref_parts[0]),
                            ("contrastive", (p0[1] + p1[1]) / 2, ref_parts[1])):
        print(f"[coca dp] {case} {name}: {got:.6f} against {want:.6f}")
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
            print(f"[coca dp] {case} grad {name}: {err:.2e} of its largest element")
        worst = max(worst, (name, err), key=lambda x: x[1])
        assert err < 2e-2, (name, err)
    print(f"[coca dp] {case}: {len(compared)} of {len(names)} parameters compared, worst {worst[0]} {worst[1]:.2e}")
    assert always <= compared
