"""tests/conv_reference.py checked on the host.  The reference has to equal fp64 torch conv2d and its autograd (exactly on
`exact_operands`, to 1e-12 on ordinary ones); `exact_operands` has to pass its own `holds` assertions at every shape
tests/test_conv_kernels_gpu.py uses; a numpy model of the kernels' arithmetic -- exact fp32 products of bf16 values summed in fp32 in
several orders, partial sums folded, a round-to-nearest-even bf16 store wherever a kernel stores bf16 -- has to stay inside `bars` for
every entry-point family and to reproduce the reference bit for bit on `exact_operands`; the bars' second-rounding terms are shown to
be what the model needs; and four injected faults (a dropped product, a tap read from the neighbouring row at column 30 of a 61-wide
map, one channel's bias left out, taps t and 8 - t swapped in one group) have to be caught -- by the zero bar on exact operands, and
the first, second and fourth by the derived bars on ordinary ones, where the 2e-2-of-the-tensor's-maximum measure of
tests/test_kernels_gpu.py lets the dropped product pass.  Prints the largest error / bar per family (`-s`).  No GPU."""
import numpy as np
import pytest
import torch

import conv_reference as R
from conv_reference import Conv
from gemm_reference import np_bf16_rne
from test_gemm_reference_host import fsum

ORDERS = ("sequential", "chunks16", "pairwise")
f32 = np.float32


@pytest.fixture(scope="module")
def pools():
    g = torch.Generator().manual_seed(4711)
    return R.exact_pool(g), R.normal_pool(g)


# ------------------------------------------------------------------------------------------------ the reference against torch
TORCH_SHAPES = [Conv(2, 7, 9, 16, 24, 3, 1, 1), Conv(2, 8, 6, 16, 24, 3, 2, 1), Conv(1, 7, 8, 16, 32, 3, 1, 2), Conv(2, 6, 5, 16, 32, 3, 2, 2),
                Conv(1, 5, 4, 48, 96, 3, 1, 6), Conv(1, 4, 7, 48, 48, 3, 2, 6), Conv(2, 1, 1, 8, 8, 3, 1, 1), Conv(2, 1, 1, 8, 8, 3, 2, 1),
                Conv(1, 2, 2, 8, 16, 3, 1, 1), Conv(1, 2, 2, 8, 16, 3, 2, 1), Conv(1, 1, 5, 8, 8, 3, 2, 1), Conv(1, 6, 1, 8, 8, 3, 1, 1),
                Conv(1, 2, 7, 16, 16, 3, 2, 2), Conv(2, 3, 4, 16, 40, 1, 1, 1)]


def torch_conv(s, ops):
    x = ops["x"].double().permute(0, 3, 1, 2).requires_grad_(True)
    ci = s.C // s.groups
    w = ops["what"].double().view(s.Cout, s.k * s.k, ci).permute(0, 2, 1).reshape(s.Cout, ci, s.k, s.k).requires_grad_(True)
    b = ops["bias"].double().requires_grad_(True)
    y = torch.nn.functional.conv2d(x, w, b, stride=s.stride, padding=s.k // 2, groups=s.groups)
    y.backward(ops["dy"].double().permute(0, 3, 1, 2))
    return {"y": y.detach().permute(0, 2, 3, 1), "dx": x.grad.permute(0, 2, 3, 1),
            "dW": w.grad.view(s.Cout, ci, s.k * s.k).permute(0, 2, 1).reshape(s.Cout, s.k * s.k * ci), "dbias": b.grad + ops["dbias0"].double()}


@pytest.mark.parametrize("s", TORCH_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_reference_equals_fp64_conv2d_and_its_autograd(pools, s):
    ex, no = R.exact_operands(pools[0], s, cols=True), R.normal_operands(pools[1], s)
    for key, want in torch_conv(s, ex).items():
        assert want.shape == ex["ref"][key].shape and torch.equal(ex["ref"][key], want), (tuple(s), key)
    for key, want in torch_conv(s, no).items():
        assert float((no["ref"][key] - want).abs().max()) <= 1e-12 * float(want.abs().max()), (tuple(s), key)


def test_layout_helpers_and_the_flipped_bank():
    t = torch.arange(2 * 3 * 4 * 5, dtype=torch.float32).view(2, 3, 4, 5)
    tp = R.to_bordered(t, 7.0)
    assert tp.shape == (2, 5, 6, 5) and torch.equal(R.interior(tp), t) and float(tp[:, 0].min()) == 7.0 and float(tp[:, :, -1].max()) == 7.0
    assert int((tp == 7.0).sum()) == tp.numel() - t.numel() + int((t == 7.0).sum())
    g, ci, co = 2, 3, 5
    what = torch.randn(g * co, 9 * ci)
    wt = R.flipped_bank(what, g * ci, g * co, g)
    assert wt.shape == (g * ci, 9 * co)
    for grp, c, t9, o in ((0, 0, 0, 0), (1, 2, 3, 4), (1, 0, 8, 2), (0, 1, 4, 3)):
        assert wt[grp * ci + c, (8 - t9) * co + o] == what[grp * co + o, t9 * ci + c]
    # the data gradient IS the forward of dy with that bank: the same reference, the roles of x and dy exchanged
    s = Conv(1, 4, 5, g * ci, g * co, 3, 1, g)
    gen = torch.Generator().manual_seed(5)
    ops = {"x": torch.randn((1, 4, 5, g * ci), generator=gen), "what": what, "dy": torch.randn((1, 4, 5, g * co), generator=gen),
           "bias": torch.zeros(g * co), "dbias0": torch.zeros(g * co)}
    back = Conv(1, 4, 5, g * co, g * ci, 3, 1, g)
    fwd_of_dy = R.reference(back, {"x": ops["dy"], "what": wt, "dy": ops["x"], "bias": torch.zeros(g * ci), "dbias0": torch.zeros(g * ci)})["y"]
    assert float((fwd_of_dy - R.reference(s, ops)["dx"]).abs().max()) < 1e-12


# ------------------------------------------------------------------------------------------------ exact operands at the GPU file's shapes
@pytest.mark.parametrize("s", list(dict.fromkeys(R.GPU_SHAPES)), ids=lambda s: "x".join(map(str, s)))
def test_exact_operands_hold_at_every_gpu_shape(pools, s):
    ex = R.exact_operands(pools[0], s, cols=s in R.NHWC_SHAPES)
    bar = R.bars(s, ex, exact=True)
    assert all(float(b.max()) == 0.0 for b in bar.values())
    assert float(ex["ref"]["y"].abs().max()) <= 256 and float(ex["ref"]["dx"].abs().max()) <= 256


def test_exact_operands_refuses_sums_the_type_cannot_hold(pools):
    epool = dict(pools[0])
    epool["x"] = torch.ones_like(epool["x"])
    epool["what"] = torch.ones_like(epool["what"])
    with pytest.raises(AssertionError):
        R.exact_operands(epool, Conv(1, 3, 3, 64, 64, 3, 1, 1))           # y = 576 in the middle: no bf16 number
    ex = R.exact_operands(torch.Generator().manual_seed(1), Conv(1, 3, 3, 8, 8, 3, 1, 1))
    assert ex["x"].shape == (1, 3, 3, 8) and ex["ref"]["y"].shape == (1, 3, 3, 8)


# ------------------------------------------------------------------------------------------------ the model of the kernels' rounding
def npy(t):
    return t.cpu().numpy().astype(f32)


def patches(s, x):
    """[B, Ho, Wo, g, kk, ci]: the input pixel every (output pixel, tap) reads, zeros outside the image"""
    B, H, W, C = x.shape
    g, pad = s.groups, s.k // 2
    Ho, Wo = R.out_hw(s)
    xp = np.zeros((B, H + 2 * pad, W + 2 * pad, g, C // g), f32)
    xp[:, pad:pad + H, pad:pad + W] = x.reshape(B, H, W, g, C // g)
    out = np.zeros((B, Ho, Wo, g, s.k * s.k, C // g), f32)
    for t in range(s.k * s.k):
        ky, kx = divmod(t, s.k)
        out[:, :, :, :, t] = xp[:, ky:ky + s.stride * (Ho - 1) + 1:s.stride, kx:kx + s.stride * (Wo - 1) + 1:s.stride]
    return out


def dx_products(s, what, dy):
    """[B, H + 2p, W + 2p, g, ci, kk, co]: every product dy * w at the (padded) input pixel it is added to, zeros where a tap has none"""
    B, Ho, Wo, _ = dy.shape
    g, kk, pad = s.groups, s.k * s.k, s.k // 2
    ci, co = s.C // g, s.Cout // g
    wg, dyg = what.reshape(g, co, kk, ci), dy.reshape(B, Ho, Wo, g, co)
    P = np.zeros((B, s.H + 2 * pad, s.W + 2 * pad, g, ci, kk, co), f32)
    for t in range(kk):
        ky, kx = divmod(t, s.k)
        P[:, ky:ky + s.stride * (Ho - 1) + 1:s.stride, kx:kx + s.stride * (Wo - 1) + 1:s.stride, :, :, t] = (
            dyg[:, :, :, :, None, :] * wg[:, :, t].transpose(0, 2, 1)[None, None, None])
    return P


def model(s, ops, order="sequential", dx="gemm", folds=1, drop=None, cols_store=np_bf16_rne, slice_store=np_bf16_rne):
    """y, dx, dW, dbias of shape `s` as the kernels of its family compute them, as fp64 torch tensors.  drop = a flat index into the
    products of y that is left out."""
    x, what, dy, bias, prior = (npy(ops[k]) for k in ("x", "what", "dy", "bias", "dbias0"))
    B, H, W, C = x.shape
    g, kk, pad = s.groups, s.k * s.k, s.k // 2
    ci, co = C // g, s.Cout // g
    Ho, Wo = R.out_hw(s)
    cols = patches(s, x)
    wg = what.reshape(g, co, kk * ci)
    out = {}
    P = cols.reshape(B, Ho, Wo, g, 1, kk * ci) * wg[None, None, None]                       # [B, Ho, Wo, g, co, K]
    if drop is not None:
        P.reshape(-1)[drop] = 0.0
    out["y"] = np_bf16_rne(fsum(P, order).reshape(B, Ho, Wo, s.Cout) + bias)
    inner = (slice(None), slice(pad, pad + H), slice(pad, pad + W))
    if dx == "gemm":
        Pd = dx_products(s, what, dy)
        out["dx"] = np_bf16_rne(fsum(Pd.reshape(Pd.shape[:5] + (-1,)), order)[inner].reshape(B, H, W, C))
    elif dx == "cols":
        dcols = cols_store(fsum(dx_products(s, what, dy), order))                          # [.., g, ci, 9]: one stored entry per tap
        out["dx"] = np_bf16_rne(fsum(dcols, "sequential")[inner].reshape(B, H, W, C))     # col2im3_kernel: t = 0 .. 8 in turn
    else:
        one = Conv(s.B, s.H, s.W, 64, 64, 3, 2, 1)
        v = None
        for i in range(R.shared_slices(s)):
            Pd = dx_products(one, what[64 * i:64 * i + 64], np.ascontiguousarray(dy[..., 64 * i:64 * i + 64]))
            part = fsum(Pd.reshape(Pd.shape[:5] + (-1,)), order)[inner].reshape(B, H, W, C)
            v = part if v is None else v + part
            v = slice_store(v) if i + 1 < R.shared_slices(s) else np_bf16_rne(v)
        out["dx"] = v
    # weight gradient: the pixels dealt to `folds` partial sums (banks, or k-slabs), each summed on its own, folded one after the other
    px = B * Ho * Wo
    dyf, cf = dy.reshape(px, g, co), cols.reshape(px, g, kk * ci)
    bounds = [px * i // folds for i in range(folds + 1)]
    parts, bparts = [], []
    for a, b in zip(bounds[:-1], bounds[1:]):
        PW = dyf[a:b].transpose(1, 2, 0)[:, :, None, :] * cf[a:b].transpose(1, 2, 0)[:, None, :, :]   # [g, co, K, pixels]
        parts.append(fsum(PW, order))
        bparts.append(fsum(dyf[a:b].transpose(1, 2, 0), order))
    out["dW"] = fsum(np.stack(parts, -1), "sequential").reshape(s.Cout, kk * ci)
    out["dbias"] = fsum(np.stack(bparts, -1), "sequential").reshape(s.Cout) + prior
    return {k: torch.from_numpy(np.ascontiguousarray(v)).to(R.F64) for k, v in out.items()}


# (family, shape, how dx is formed, the fold counts modelled): real channel counts per group on maps of a few pixels
MODEL_CASES = [("direct / view 64->64", Conv(2, 3, 4, 64, 64, 3, 1, 1), "gemm", (1, 3, 24)),
               ("direct / view 16->32 x 2 groups", Conv(1, 4, 5, 32, 64, 3, 1, 2), "gemm", (1, 7)),
               ("stride 2, 64->64 x 2 groups", Conv(1, 5, 4, 128, 128, 3, 2, 2), "gemm", (1, 6)),
               ("stride 2, shared input 64->128", Conv(1, 5, 4, 64, 128, 3, 2, 1), "slices", (1, 6)),
               ("stride 2, shared input 64->192", Conv(2, 3, 3, 64, 192, 3, 2, 1), "slices", (1,)),
               ("nhwc k=3", Conv(2, 3, 4, 64, 64, 3, 1, 1), "cols", (1, 2)),
               ("nhwc k=3 stride 2, Cg = 8", Conv(1, 5, 6, 16, 32, 3, 2, 2), "cols", (1, 5)),
               ("nhwc k=3 co = 512", Conv(1, 3, 2, 8, 512, 3, 2, 1), "cols", (1,)),
               ("nhwc k=1", Conv(2, 3, 4, 64, 96, 1, 1, 1), "gemm", (1, 4))]


def test_model_stays_inside_the_bars_and_is_exact_on_exact_operands(pools):
    worst = {}
    for name, s, dx, fold_counts in MODEL_CASES:
        ex, no = R.exact_operands(pools[0], s, cols=dx == "cols"), R.normal_operands(pools[1], s)
        Ho, Wo = R.out_hw(s)
        for folds in fold_counts:
            ebar = R.bars(s, ex, dx, L=s.B * Ho * Wo, folds=folds, exact=True)
            nbar = R.bars(s, no, dx, L=s.B * Ho * Wo, folds=folds)
            for order in ORDERS:
                got = model(s, ex, order, dx, folds)
                for key, want in ex["ref"].items():
                    assert float(ebar[key].max()) == 0.0
                    assert torch.equal(got[key], want), (name, folds, order, key, R.first_bad_nd(got[key], want, ebar[key]))
                got = model(s, no, order, dx, folds)
                for key, want in no["ref"].items():
                    bad = R.first_bad_nd(got[key], want, nbar[key])
                    assert bad is None, (name, folds, order, key, bad)
                    tag = (name, key)
                    worst[tag] = max(worst.get(tag, 0.0), R.worst_ratio(got[key], want, nbar[key]))
    for (name, key), r in sorted(worst.items()):
        print("model  %-34s %-5s  worst error / bar %.3f" % (name, key, r))
    assert worst and max(worst.values()) < 1.0


def test_cols_bar_needs_the_dcols_store_term(pools):
    """ia_conv_nhwc_bwd_data stores the nine dcols entries as bf16 before col2im3_kernel adds them.  A model that keeps them in fp32
    stays inside the bar WITHOUT that term; the model of what the kernels do (a bf16 store per entry) does not, and stays inside the
    bar with it."""
    s = Conv(2, 5, 6, 64, 64, 3, 1, 1)
    no = R.normal_operands(pools[1], s)
    L = s.B * s.H * s.W
    bar, without = R.bars(s, no, "cols", L=L)["dx"], R.bars(s, no, "cols", L=L, without="cols_store")["dx"]
    want = no["ref"]["dx"]
    kept, stored = model(s, no, dx="cols", cols_store=lambda v: v)["dx"], model(s, no, dx="cols")["dx"]
    print("dcols store: fp32 entries %.3f of the bar without the term; bf16 entries %.3f of it, %.3f of the bar with the term" % (
        R.worst_ratio(kept, want, without), R.worst_ratio(stored, want, without), R.worst_ratio(stored, want, bar)))
    assert R.first_bad_nd(kept, want, without) is None
    assert R.first_bad_nd(stored, want, without) is not None
    assert R.first_bad_nd(stored, want, bar) is None


def test_slices_bar_needs_the_per_slice_store_term(pools):
    """the shared-input data gradient stores dx as bf16 after every 64-channel slice of dy and reads it back for the next"""
    s = Conv(2, 7, 6, 64, 192, 3, 2, 1)
    no = R.normal_operands(pools[1], s)
    L = s.B * 4 * 3
    bar, without = R.bars(s, no, "slices", L=L)["dx"], R.bars(s, no, "slices", L=L, without="slice_store")["dx"]
    want = no["ref"]["dx"]
    kept, stored = model(s, no, dx="slices", slice_store=lambda v: v)["dx"], model(s, no, dx="slices")["dx"]
    print("slice store: fp32 running sum %.3f of the bar without the term; bf16 running sum %.3f of it, %.3f of the bar with the term" % (
        R.worst_ratio(kept, want, without), R.worst_ratio(stored, want, without), R.worst_ratio(stored, want, bar)))
    assert R.first_bad_nd(kept, want, without) is None
    assert R.first_bad_nd(stored, want, without) is not None
    assert R.first_bad_nd(stored, want, bar) is None


def test_fold_term_counts_the_adds_of_the_fold(pools):
    """The weight gradients fold partial sums (k-slabs, per-workgroup banks): every bank is one more add.  Where L counts the pixels a
    kernel really adds -- the terms of ALL banks together -- the folds re-order the same sum and the any-order bound (L + 2) * U already
    holds them; the term is needed where the banks' own sums are shorter than the adds that follow them.  The sharpest such case: every
    bank holds ONE pixel (a product of two bf16 numbers is exact in fp32, so a bank carries no error at all) and the whole error is the
    fold's.  The bar then has to be the bound of a sum of `folds` terms: with L = 1 (the length of a bank's sum) it is
    (1 + 2 + folds + 1) * U with the term and 3 * U, whatever the number of banks, without it -- which a sequential fold of 3000 banks
    breaks."""
    folds = 3000
    g = torch.Generator().manual_seed(77)
    dy = (torch.rand((folds,), generator=g) + 0.5).to(torch.bfloat16).to(torch.float32)
    x = (torch.rand((folds,), generator=g) + 0.5).to(torch.bfloat16).to(torch.float32)
    s = Conv(folds, 1, 1, 8, 8, 1, 1, 1)
    ops = {"x": x.view(folds, 1, 1, 1).expand(folds, 1, 1, 8).contiguous(), "dy": dy.view(folds, 1, 1, 1).expand(folds, 1, 1, 8).contiguous(),
           "what": torch.zeros(8, 8), "bias": torch.zeros(8), "dbias0": torch.zeros(8)}
    ops["ref"] = R.reference(s, ops)
    got = model(s, ops, "sequential", folds=folds)
    bar, without = R.bars(s, ops, L=1, folds=folds), R.bars(s, ops, L=1, folds=folds, without="fold")
    for key in ("dW", "dbias"):
        print("fold of %d one-pixel banks, %-5s: %.3f of the bar with the term, %.3f of the bar without it" % (
            folds, key, R.worst_ratio(got[key], ops["ref"][key], bar[key]), R.worst_ratio(got[key], ops["ref"][key], without[key])))
        assert R.first_bad_nd(got[key], ops["ref"][key], bar[key]) is None
    assert any(R.first_bad_nd(got[key], ops["ref"][key], without[key]) is not None for key in ("dW", "dbias"))


# ------------------------------------------------------------------------------------------------ injected faults
FAULT_SHAPE = Conv(1, 9, 61, 128, 128, 3, 1, 2)


def faulty(s, ops, fault):
    """the reference y of `s` with one fault of a subtly wrong kernel applied; returns (y', the pixels / channels it may differ at)"""
    x, what, bias = R.d(ops["x"]), R.d(ops["what"]), R.d(ops["bias"])
    y = ops["ref"]["y"].clone()
    ci, co = s.C // s.groups, s.Cout // s.groups
    xp = torch.zeros((s.B, s.H + 3, s.W + 2, s.C), dtype=R.F64)
    xp[:, 1:s.H + 1, 1:s.W + 1] = x
    if fault == "dropped product":
        # one x * w of output (0, 4, 17, channel 70): the one of median size among that element's non-zero products
        b, oy, ox, o = 0, 4, 17, 70
        grp = o // co
        prods = torch.stack([xp[b, oy + t // 3, ox + t % 3, grp * ci:(grp + 1) * ci] * what[o, t * ci:(t + 1) * ci] for t in range(9)]).reshape(-1)
        nz = torch.nonzero(prods).reshape(-1)
        pick = nz[torch.argsort(prods[nz].abs())[nz.numel() // 2]]
        y[b, oy, ox, o] -= prods[pick]
        return y, float(prods[pick])
    if fault == "halo from the neighbouring row":
        # tap 5 (ky 1, kx 2) of output column 30 -- the first column of the second 30-wide tile -- reads one row too low, in group 1
        t, ox, grp = 5, 30, 1
        w_t = what[grp * co:(grp + 1) * co, t * ci:(t + 1) * ci]
        right = xp[:, 1:s.H + 1, ox + 2, grp * ci:(grp + 1) * ci]
        wrong = xp[:, 2:s.H + 2, ox + 2, grp * ci:(grp + 1) * ci]
        y[:, :, ox, grp * co:(grp + 1) * co] += (wrong - right) @ w_t.t()
        return y, None
    if fault == "bias left out":
        o = int(torch.nonzero(bias)[3])
        y[..., o] -= bias[o]
        return y, None
    assert fault == "taps swapped"
    w2 = what.clone().view(s.groups, co, 9, ci)
    w2[1, :, [2, 6]] = w2[1, :, [6, 2]]
    return R.reference(s, dict(ops, what=w2.view(s.Cout, 9 * ci)))["y"], None


@pytest.mark.parametrize("fault", ["dropped product", "halo from the neighbouring row", "bias left out", "taps swapped"])
def test_injected_faults_are_caught(pools, fault):
    s = FAULT_SHAPE
    ex, no = R.exact_operands(pools[0], s), R.normal_operands(pools[1], s)
    got, _ = faulty(s, ex, fault)
    bad = R.first_bad_nd(got, ex["ref"]["y"], R.bars(s, ex, exact=True)["y"])
    assert bad is not None, fault
    print("%-32s exact operands: %s" % (fault, bad))
    got, size = faulty(s, no, fault)
    bar = R.bars(s, no, L=s.B * (s.H + 2) * (s.W + 2))["y"]
    bad = R.first_bad_nd(got, no["ref"]["y"], bar)
    ratio = R.worst_ratio(got, no["ref"]["y"], bar)
    old = float((got - no["ref"]["y"]).abs().max() / no["ref"]["y"].abs().max())       # rel_err of tests/test_kernels_gpu.py
    print("%-32s ordinary operands: %.1f x the bar; max|a - b| / max|b| = %.2e (the older tests allow 2e-2)" % (fault, ratio, old))
    if fault != "bias left out":
        assert bad is not None, fault
    if fault == "dropped product":
        assert old < 2e-2 and abs(size) > 0.02, (old, size)     # a product of ordinary size, and the coarse measure lets it through
