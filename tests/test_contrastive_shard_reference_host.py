"""tests/contrastive_shard_reference.py has to be right before the GPU test compares the shard kernels with it.  In fp64 on the CPU:
  * for several splits of one global batch -- unequal ones among them -- the mean of the shard losses, the stacked shard gradients
    / world and the summed dlog_scale / world are the values of the square reference (contrastive_reference.forward / backward) on the
    whole batch: the invariant the data-parallel step rests on;
  * a CPU model of the kernels' fp32 chains (four accumulators in k order, lane l taking terms l, l + 64, ..., then a tree over the
    lanes) stays inside the bounds, and two injected faults -- the diagonal taken at i instead of row_offset + i, c without the
    `world` factor -- fall outside them: the bounds are neither too tight for correct arithmetic nor loose enough to hide a wrong index.
"""
import math

import numpy as np
import pytest
import torch

import contrastive_reference as R
import contrastive_shard_reference as S

F64, F32 = torch.float64, torch.float32
DLOSS = 0.75
SPLITS = [(4, 4), (3, 1, 7), (1, 64), (17, 48), (3, 17, 45), (5,)]


def agree(name, got, want, rel=1e-11):
    tol = rel * max(1.0, float(want.abs().max()))
    assert float((got - want).abs().max()) <= tol, (name, float((got - want).abs().max()), tol)


@pytest.mark.parametrize("kind", R.KINDS)
@pytest.mark.parametrize("split", SPLITS, ids=lambda s: "+".join(map(str, s)))
def test_shards_assemble_to_the_global_batch(split, kind):
    G, W, H = sum(split), len(split), 64
    t, im = R.build(G, H, kind, seed=11 + G)
    for log_scale in (0.0, 1.0):
        glob = R.forward(t, im, log_scale)
        gb = R.backward(t, im, log_scale, dloss=DLOSS, fwd=glob)
        o, losses, dts, dis, dls = 0, [], [], [], 0.0
        for B in split:
            f = S.forward(t, im, log_scale, o, B, W)
            b = S.backward(t, im, log_scale, o, B, W, dloss=DLOSS, fwd=f, glob=glob)
            agree("sim_t", f["sim_t"], glob["sim"][o:o + B])
            agree("sim_i", f["sim_i"], glob["sim"][:, o:o + B].T)
            agree("lse_row_l", f["lse_row_l"], glob["lse_row"][o:o + B])
            agree("lse_col_l", f["lse_col_l"], glob["lse_col"][o:o + B])
            for k in ("sim_t_bound", "sim_i_bound", "lse_row_l_bound", "lse_col_l_bound", "loss_bound"):
                assert (f[k] > 0).all() and torch.isfinite(f[k]).all(), k
            for k in ("Gt_bound", "Gi_bound", "dtext_l_bound", "dimage_l_bound", "dlog_scale_bound"):
                assert (b[k] > 0).all() and torch.isfinite(b[k]).all(), k
            losses.append(f["loss"]); dts.append(b["dtext_l"]); dis.append(b["dimage_l"]); dls = dls + b["dlog_scale"]
            o += B
        agree("loss", torch.stack(losses).mean(), glob["loss"])
        # the gradients cancel from terms of the size of |G| |sim|: the agreement is relative to those
        agree("dtext", torch.cat(dts) / W, gb["dtext"], rel=1e-9)
        agree("dimage", torch.cat(dis) / W, gb["dimage"], rel=1e-9)
        scale = max(1.0, float((gb["G"] * glob["sim"]).abs().sum()))
        assert abs(float(dls) / W - float(gb["dlog_scale"])) <= 1e-11 * scale


def test_world_one_is_the_square_reference():
    t, im = R.build(17, 192, "random", seed=5)
    glob = R.forward(t, im, 1.0)
    gb = R.backward(t, im, 1.0, dloss=DLOSS, fwd=glob)
    f = S.forward(t, im, 1.0, 0, 17, 1)
    b = S.backward(t, im, 1.0, 0, 17, 1, dloss=DLOSS, fwd=f, glob=glob)
    agree("loss", f["loss"], glob["loss"])
    agree("Gt", b["Gt"], gb["G"]); agree("Gi", b["Gi"], gb["G"].T)
    agree("dtext", b["dtext_l"], gb["dtext"]); agree("dimage", b["dimage_l"], gb["dimage"])
    assert abs(float(b["dlog_scale"] - gb["dlog_scale"])) <= 1e-11
    # the bounds are the square reference's where the chains are: only den's rounding is added
    assert torch.equal(f["sim_t_bound"], glob["sim_bound"]) and torch.allclose(f["lse_row_l_bound"], glob["lse_row_bound"], rtol=1e-12)
    assert float(glob["loss_bound"]) <= float(f["loss_bound"]) <= 1.2 * float(glob["loss_bound"])


def test_accumulated_value_is_added():
    t, im = R.build(7, 128, "random", seed=4)
    a = S.backward(t, im, 0.0, 4, 3, 2, dloss=DLOSS)
    b = S.backward(t, im, 0.0, 4, 3, 2, dloss=DLOSS, accumulated_onto=2.5)
    assert float(b["dlog_scale"]) == float(a["dlog_scale"]) + 2.5


def test_shapes_are_the_issue_s():
    assert (64, 128, 64, 768) in S.SHAPES and (1, 257, 256, 128) in S.SHAPES and len(S.SHAPES) == 8
    for B, G, o, H in S.SHAPES:
        assert B >= 1 and 0 <= o and o + B <= G and S.world_of(B, G) >= 1
    assert S.world_of(1, 1) == 1 and S.world_of(64, 128) == 2 and S.world_of(17, 65) == 4


# ------------------------------------------------------------------------------------------------ the fp32 model of the kernels
def fma32(a, b, c):
    """fmaf on fp32 values: the product is exact in fp64"""
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32)


def dot4(a, b):
    """[m, n] x [p, n] -> [m, p]: term k into accumulator k % 4 by fmaf, in k order, combined as (a0 + a1) + (a2 + a3)"""
    acc = [np.zeros((a.shape[0], b.shape[0]), np.float32) for _ in range(4)]
    for k in range(a.shape[1]):
        acc[k % 4] = fma32(a[:, k:k + 1], b[:, k][None, :], acc[k % 4])
    return (acc[0] + acc[1]) + (acc[2] + acc[3])


def wave_sum_rows(x, fma_with=None):
    """[m, n] -> [m]: lane l takes terms l, l + 64, ... in order (x, or fmaf(x, fma_with, acc)), then a tree over the 64 lanes"""
    m, n = x.shape
    lanes = np.zeros((m, 64), np.float32)
    for j in range(n):
        l = j % 64
        lanes[:, l] = lanes[:, l] + x[:, j] if fma_with is None else fma32(x[:, j], fma_with[:, j], lanes[:, l])
    w = 64
    while w > 1:
        w //= 2
        lanes = lanes[:, :w] + lanes[:, w:2 * w]
    return lanes[:, 0]


def exp32(x):
    """expf of an fp32 argument, correctly rounded (the kernels' expf is within 1 ulp)"""
    return np.exp(x.astype(np.float32).astype(np.float64)).astype(np.float32)


def lse32(x):
    m = x.max(axis=1)
    e = exp32(x - m[:, None])
    return m + np.log(wave_sum_rows(e).astype(np.float64)).astype(np.float32)


def model_forward(t, im, log_scale, o, B, world, fault=None):
    tg, ig = t.numpy(), im.numpy()
    G = tg.shape[0]
    s = exp32(np.float32(log_scale))
    sim_t, sim_i = s * dot4(tg[o:o + B], ig), s * dot4(ig[o:o + B], tg)
    lse_row_l, lse_col_l = lse32(sim_t), lse32(sim_i)
    d = np.arange(B) + (0 if fault == "diagonal" else o)
    rows = np.arange(B)
    den = np.float32(G) if fault == "world" else np.float32(G) / np.float32(world)
    r = wave_sum_rows((lse_row_l - sim_t[rows, d])[None, :])[0]
    c = wave_sum_rows((lse_col_l - sim_i[rows, d])[None, :])[0]
    return dict(sim_t=sim_t, sim_i=sim_i, lse_row_l=lse_row_l, lse_col_l=lse_col_l, loss=np.float32(0.5) * (r / den + c / den))


def model_backward(t, im, log_scale, o, B, world, fwd, lse_row_g, lse_col_g, dloss, fault=None):
    tg, ig = t.numpy(), im.numpy()
    G = tg.shape[0]
    s = exp32(np.float32(log_scale))
    den = np.float32(G) if fault == "world" else np.float32(G) / np.float32(world)
    c = np.float32(dloss) * (np.float32(0.5) / den)
    two = np.zeros((B, G), np.float32)
    two[np.arange(B), np.arange(B) + (0 if fault == "diagonal" else o)] = 2.0
    out = {}
    for name, sim, own, other, src in (("dtext_l", fwd["sim_t"], lse_row_g, lse_col_g, ig), ("dimage_l", fwd["sim_i"], lse_col_g, lse_row_g, tg)):
        p, q = exp32(sim - own[o:o + B, None]), exp32(sim - other[None, :])
        M = c * ((p + q) - two)
        out[name] = s * dot4(M, np.ascontiguousarray(src.T))
        if name == "dtext_l":
            part = wave_sum_rows(M, fma_with=sim)
            out["dlog_scale"] = wave_sum_rows(part[None, :])[0]
    return out


def ratios(got, want, names):
    return {n: float((torch.from_numpy(np.atleast_1d(np.asarray(got[n]))).to(F64).reshape(-1) - want[n].reshape(-1)).abs()
                     .div(want[n + "_bound"].reshape(-1)).max()) for n in names}


def model_against_reference(B, G, o, H, kind, log_scale, fault=None):
    W = S.world_of(B, G)
    t, im = R.build(G, H, kind, seed=1000 + 7 * G + H + R.KINDS.index(kind))
    ls32 = float(torch.tensor(log_scale, dtype=F32))
    glob = R.forward(t, im, ls32)
    f = S.forward(t, im, ls32, o, B, W)
    b = S.backward(t, im, ls32, o, B, W, dloss=DLOSS, fwd=f, glob=glob)
    # the gathered lse vectors as fp32 kernels would have produced them: rows of the whole batch through the same model
    whole = model_forward(t, im, log_scale, 0, G, 1)
    mf = model_forward(t, im, log_scale, o, B, W, fault=fault)
    mb = model_backward(t, im, log_scale, o, B, W, mf, whole["lse_row_l"], whole["lse_col_l"], DLOSS, fault=fault)
    out = ratios(mf, f, ("sim_t", "sim_i", "lse_row_l", "lse_col_l", "loss"))
    out.update(ratios(mb, b, ("dtext_l", "dimage_l", "dlog_scale")))
    return out


HOST_SHAPES = [s for s in S.SHAPES if s[3] <= 192]      # the 768-wide shape is the GPU test's: the model walks k in Python


@pytest.mark.parametrize("kind", R.KINDS)
@pytest.mark.parametrize("B,G,o,H", HOST_SHAPES)
def test_fp32_model_of_the_chains_stays_inside_the_bounds(B, G, o, H, kind):
    for log_scale in (0.0, 4.6):
        got = model_against_reference(B, G, o, H, kind, log_scale)
        assert all(math.isfinite(v) and v <= 1.0 for v in got.values()), (log_scale, got)


@pytest.mark.parametrize("B,G,o,H", [(3, 7, 4, 128), (17, 65, 48, 192), (16, 257, 100, 128)])
def test_injected_faults_fall_outside_the_bounds(B, G, o, H):
    wrong = model_against_reference(B, G, o, H, "random", 1.0, fault="diagonal")
    assert wrong["loss"] > 1.0 and wrong["dtext_l"] > 1.0 and wrong["dimage_l"] > 1.0 and wrong["dlog_scale"] > 1.0, wrong
    assert max(wrong[k] for k in ("sim_t", "sim_i", "lse_row_l", "lse_col_l")) <= 1.0      # the fault is not in those
    wrong = model_against_reference(B, G, o, H, "random", 1.0, fault="world")
    assert wrong["loss"] > 1.0 and wrong["dtext_l"] > 1.0 and wrong["dimage_l"] > 1.0 and wrong["dlog_scale"] > 1.0, wrong
