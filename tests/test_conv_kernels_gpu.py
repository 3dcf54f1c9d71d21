"""The convolution entry points of csrc/conv.hip through the C ABI against the fp64 reference of tests/conv_reference.py, ELEMENT BY
ELEMENT: ia_conv3x3_padded_fwd / _bwd_data_t / _bwd_data / _bwd_weight on the direct kernels and on the shifted-view / grouped GEMM
(ia_gemm_view), ia_conv3x3_flip_weights, ia_conv3x3_s2_padded_fwd / _bwd_weight / _bwd_data_t, and the patch-matrix path
ia_conv_nhwc_fwd / _bwd_data / _bwd_weight.

Two kinds of operands per case: `exact_operands`, on which every output is a number its type holds exactly in any summation order --
there got == reference on every element of every output, so a product dropped or doubled at a tile corner, a halo pixel taken from the
neighbouring row, one channel's bias or a wrong element in an absent tap slot shows as a whole unit -- and ordinary ones (randn), held
to the derived per-element bars of conv_reference.bars (checked on the host against a CPU model of the kernels' rounding by
tests/test_conv_reference_host.py, never fitted to a GPU result).

Every operand sits in the middle of a NaN-filled buffer (64 Ki elements before and after): the direct kernels' last tiles reach past the
tensor, what they find there must be the range-check zeros, and a NaN in an output is a read outside the operand.  Outputs are
pre-filled with a sentinel bf16 holds; the guards behind every output, the whole border where the header says it is not written (the
direct and the stride-2 kernels; the view GEMM "carries garbage in its border rows"), WS_TAIL bytes behind the stated workspace size
and every input have to come back bit-unchanged.  dbias is += and starts from a whole-number (or random) prior, dW is overwritten
and starts from NaN, dy's border is NaN where the header says it is not read (the stride-2 weight gradient) and zero where it asks for
zeros.

Each case ASSERTS the path it is meant for from what the library exports (ia_conv3x3_direct_supported, ia_conv3x3_s2_supported, the
pixel count against IA_CONV_DIRECT_WGRAD_MIN); the weight gradient runs on both of its paths at every direct-capable shape, each path
twice, bit-identical.  `folds`, the number of partial sums a weight gradient folds, is bounded from the exported workspace sizes: a
split-K slab or a per-workgroup bank takes Cout * (K + 1) floats there.  Every comparison prints max error / bar (`-s` shows them).

Worst error / bar seen on one MI355X over all cases, ordinary operands (recorded figures, no input to any bar; on the exact operands
every output of every case was equal on every element).  A correctly rounded bf16 store alone reaches 1.0 of its 2^-8 allowance just
above a power of two, so the bf16 outputs sit where they should:
  ia_conv3x3_padded_fwd               direct          y 0.987     view GEMM   y 0.980
  ia_conv3x3_padded_bwd_data_t        direct          dx 0.968
  ia_conv3x3_padded_bwd_data          view GEMM       dx 0.980
  ia_conv3x3_padded_bwd_weight        direct          dW 0.003  dbias 0.005     split-K view GEMM   dW 0.008  dbias 0.065
  ia_conv3x3_s2_padded_fwd                            y 0.923
  ia_conv3x3_s2_padded_bwd_data_t                     dx 0.950    shared input  dx 0.888
  ia_conv3x3_s2_padded_bwd_weight                     dW 0.004  dbias 0.104
  ia_conv_nhwc_fwd                    k = 3           y 0.983     k = 1       y 0.982
  ia_conv_nhwc_bwd_data               k = 3           dx 0.831    k = 1       dx 0.924
  ia_conv_nhwc_bwd_weight             k = 3           dW 0.060  dbias 0.043     k = 1   dW 0.023  dbias 0.012
The fp32 bars of dW and dbias are loose by construction: they grow with the number of pixels L (and of folded banks, bounded by up to
512 / groups), the error of a sum of random signs with sqrt(L).  At 0.003 - 0.008 the dW bar of the direct and the stride-2 kernels
still holds a single dropped dy * x product (a product of median size is 3.7 bars at 2 x 9 x 31 x 64 -> 64), nothing finer; what is
sharp for these outputs is the equality on the exact operands.
"""
import pytest
import torch

import conv_reference as R

pytestmark = pytest.mark.gpu

F64, F32, BF16 = torch.float64, torch.float32, torch.bfloat16
GUARD = 65536          # elements of NaN (inputs) or sentinel (outputs) before and after every tensor: >= 64 KiB in every type
SENT = 768.0           # sentinel of the outputs (exact in bf16)
NAN = float("nan")
WS_TAIL = 256          # bytes behind the stated workspace size that have to stay untouched
WGRAD_MIN = 100000     # pixels from which ia_conv3x3_padded_bwd_weight takes its direct kernel (IA_CONV_DIRECT_WGRAD_MIN unset)
TH, TW = 8, 30         # the direct kernels' output tile
IA_ERR_ARG, IA_ERR_WORKSPACE, IA_ERR_UNSUPPORTED = -1, -3, -4
RATIOS = {}


@pytest.fixture(scope="module")
def lib(gpu):
    from item_alignment_amd import _lib
    return _lib.load()


@pytest.fixture(scope="module")
def pools(gpu):
    """every draw of the module, once, on the device"""
    g = torch.Generator(device="cuda").manual_seed(9035)
    return R.exact_pool(g), R.normal_pool(g)


def sp():
    from item_alignment_amd import _lib
    return _lib.stream_ptr()


def ok(rc, what):
    from item_alignment_amd import _lib
    _lib.check(rc, what)


def bits(t):
    return t.view(torch.int16 if t.dtype == BF16 else torch.int32 if t.dtype == F32 else torch.uint8)


class Buf:
    """a tensor in the middle of a guard-filled buffer; remembers its bits"""

    def __init__(self, shape, dtype, guard, fill=None, data=None):
        n = 1
        for v in shape:
            n *= v
        self.n = n
        self.whole = torch.full((n + 2 * GUARD,), guard, dtype=dtype, device="cuda")
        self.v = self.whole[GUARD:GUARD + n].view(shape)
        if fill is not None:
            self.v.fill_(fill)
        if data is not None:
            self.v.copy_(data)
        self.before = self.whole.clone()

    def ptr(self):
        return self.v.data_ptr()

    def unchanged(self, what):
        assert torch.equal(bits(self.whole), bits(self.before)), what + " was written"

    def guards_unchanged(self, what):
        a, b = bits(self.whole), bits(self.before)
        assert torch.equal(a[:GUARD], b[:GUARD]) and torch.equal(a[GUARD + self.n:], b[GUARD + self.n:]), what + ": written outside the tensor"

    def border_unchanged(self, what):
        """bordered [B, H + 2, W + 2, C]: everything but the interior"""
        self.guards_unchanged(what)
        a, b = bits(self.v).clone(), bits(self.before[GUARD:GUARD + self.n].view(self.v.shape)).clone()
        a[:, 1:-1, 1:-1] = 0
        b[:, 1:-1, 1:-1] = 0
        assert torch.equal(a, b), what + ": the border was written"


def inp(t, dtype=BF16):
    return Buf(tuple(t.shape), dtype, NAN, data=t.to(dtype))


def workspace(nbytes):
    return torch.full((max(nbytes, 16) + WS_TAIL,), 0x5A, dtype=torch.uint8, device="cuda")


def ws_tail_ok(ws, nbytes, what):
    assert bool((ws[max(nbytes, 16):] == 0x5A).all()), what + ": the workspace was written past its stated size"


def verdict(entry, key, where, got, want, bar, exact):
    g64 = got.to(F64)
    ratio = R.worst_ratio(g64, want, bar)
    if exact:
        assert float(bar.max()) == 0.0
    else:
        RATIOS[(entry, key)] = max(RATIOS.get((entry, key), 0.0), ratio)
        print("%-34s %-5s %-44s worst error / bar %.3f" % (entry, key, where, ratio))
    bad = R.first_bad_nd(g64, want, bar)
    assert bad is None, "%s %s %s (%s operands): %s" % (entry, key, where, "exact" if exact else "ordinary", bad)


def report():
    for (entry, key), r in sorted(RATIOS.items()):
        print("worst so far  %-34s %-5s error / bar %.3f" % (entry, key, r))


def tiles(H, W):
    return (H + TH - 1) // TH, (W + TW - 1) // TW


def folds_bound(wsb, Cout, K):
    """an upper bound of the partial sums a weight gradient folds: each (k-slab or workgroup bank) takes Cout * (K + 1) floats of the
    workspace the library asks for"""
    return max(1, wsb // (Cout * (K + 1) * 4))


def operands(pools, s, exact, cols=False):
    return R.exact_operands(pools[0], s, "cuda", cols=cols) if exact else R.normal_operands(pools[1], s, "cuda")


# ------------------------------------------------------------------------------------------------------------------ stride 1, bordered
def flip(lib, what, Cin, Cout, groups):
    """ia_conv3x3_flip_weights, checked against the reference bank"""
    src = inp(what)
    dst = Buf((Cin, 9 * (Cout // groups)), BF16, NAN, fill=SENT)       # (NaN around it: it is the next kernel's input)
    ok(lib.ia_conv3x3_flip_weights(src.ptr(), dst.ptr(), Cin, Cout, groups, sp()), "flip")
    torch.cuda.synchronize()
    src.unchanged("flip: what")
    dst.guards_unchanged("flip: what_t")
    assert torch.equal(dst.v, R.flipped_bank(what.to(BF16), Cin, Cout, groups)), ("ia_conv3x3_flip_weights", Cin, Cout, groups)
    dst.before = dst.whole.clone()             # from here on an input
    return dst


def padded_case(lib, pools, monkeypatch, s, direct, dgrads):
    """ia_conv3x3_padded_* at shape `s`: forward, the data gradient(s) in `dgrads` ("t": direct, "view": ia_gemm_view) and the weight
    gradient on every path it has, on both kinds of operands.  direct: the forward is meant for the direct kernel."""
    B, H, W, Cin, Cout, g = s.B, s.H, s.W, s.C, s.Cout, s.groups
    ci, co = Cin // g, Cout // g
    assert ((ci, co) in R.DCONV_PAIRS and g <= 64) == direct, (tuple(s), "the forward is routed to the other kernel")
    assert bool(lib.ia_conv3x3_direct_supported(Cin, Cout, g)) == direct
    where = "x".join(map(str, (B, H, W, Cin, Cout, g)))
    wsb = lib.ia_conv3x3_padded_workspace_bytes(B, H, W, Cin, Cout, g)
    folds = folds_bound(wsb, Cout, 9 * ci)
    ty, tx = tiles(H, W)
    wpaths = [("view", B * (H + 2) * (W + 2), folds)]                # the split-K view GEMM sums every bordered row
    if (ci, co) in R.DCONV_WGRAD_PAIRS:
        # the direct kernel sums 8 x 32-pixel tiles into one bank per workgroup: at most one workgroup per tile of a group, and no more
        # banks than the workspace holds
        wpaths.append(("direct", B * ty * TH * tx * 32, min(folds, B * ty * tx)))
        assert folds >= min(B * ty * tx, 512 // g), "the workspace bound does not cover the direct kernel's banks"
    assert B * H * W < WGRAD_MIN
    for exact in (True, False):
        ops = operands(pools, s, exact)
        ref = ops["ref"]
        xp, dyp = inp(R.to_bordered(ops["x"])), inp(R.to_bordered(ops["dy"]))
        what, bias = inp(ops["what"]), inp(ops["bias"], F32)
        ins = (("xp", xp), ("dyp", dyp), ("what", what), ("bias", bias))
        bar = R.bars(s, ops, "gemm", L=1, exact=exact)
        # forward
        yp = Buf((B, H + 2, W + 2, Cout), BF16, SENT, fill=SENT)
        ok(lib.ia_conv3x3_padded_fwd(xp.ptr(), what.ptr(), bias.ptr(), yp.ptr(), B, H, W, Cin, Cout, g, sp()), "fwd")
        torch.cuda.synchronize()
        (yp.border_unchanged if direct else yp.guards_unchanged)("fwd " + where + ": yp")
        verdict("padded_fwd " + ("direct" if direct else "view"), "y", where, R.interior(yp.v), ref["y"], bar["y"], exact)
        # data gradient
        for path in dgrads:
            dxp = Buf((B, H + 2, W + 2, Cin), BF16, SENT, fill=SENT)
            if path == "t":
                what_t = flip(lib, ops["what"], Cin, Cout, g)
                ok(lib.ia_conv3x3_padded_bwd_data_t(dyp.ptr(), what_t.ptr(), dxp.ptr(), B, H, W, Cin, Cout, g, sp()), "bwd_data_t")
                torch.cuda.synchronize()
                dxp.border_unchanged("bwd_data_t " + where + ": dxp")
            else:
                ok(lib.ia_conv3x3_padded_bwd_data(dyp.ptr(), what.ptr(), dxp.ptr(), B, H, W, Cin, Cout, g, sp()), "bwd_data")
                torch.cuda.synchronize()
                dxp.guards_unchanged("bwd_data " + where + ": dxp")
            verdict("padded_bwd_data" + ("_t direct" if path == "t" else " view"), "dx", where, R.interior(dxp.v), ref["dx"], bar["dx"], exact)
        # weight + bias gradient: every path twice, bit-identical
        for path, L, nfold in wpaths:
            if path == "direct":
                monkeypatch.setenv("IA_CONV_DIRECT_WGRAD_MIN", "0")
            else:
                monkeypatch.delenv("IA_CONV_DIRECT_WGRAD_MIN", raising=False)
            wbar = R.bars(s, ops, "gemm", L=L, folds=nfold, exact=exact)
            outs = []
            for _ in range(2):
                ws = workspace(wsb)
                dW = Buf((Cout, 9 * ci), F32, SENT, fill=NAN)
                db = Buf((Cout,), F32, SENT, data=ops["dbias0"])
                ok(lib.ia_conv3x3_padded_bwd_weight(xp.ptr(), dyp.ptr(), dW.ptr(), db.ptr(), B, H, W, Cin, Cout, g, ws.data_ptr(), wsb, sp()), "bwd_weight")
                torch.cuda.synchronize()
                ws_tail_ok(ws, wsb, "bwd_weight " + where)
                dW.guards_unchanged("bwd_weight " + where + ": dW")
                db.guards_unchanged("bwd_weight " + where + ": dbias")
                outs.append((dW.v.clone(), db.v.clone()))
            assert torch.equal(bits(outs[0][0]), bits(outs[1][0])) and torch.equal(bits(outs[0][1]), bits(outs[1][1])), (where, path, "two runs differ")
            verdict("padded_bwd_weight " + path, "dW", where, outs[0][0], ref["dW"], wbar["dW"], exact)
            verdict("padded_bwd_weight " + path, "dbias", where, outs[0][1], ref["dbias"], wbar["dbias"], exact)
        monkeypatch.delenv("IA_CONV_DIRECT_WGRAD_MIN", raising=False)
        for name, b in ins:
            b.unchanged(where + ": input " + name)
    report()


@pytest.mark.parametrize("s", R.DIRECT_SHAPES + R.DIRECT_GROUP_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_direct_kernels_at_tile_edges(lib, pools, monkeypatch, s):
    """every pair of DCONV_PAIRS as a forward ((64, 32) and (32, 16) included) at 2 x 9 x 31 (one pixel past a tile in both directions),
    8 x 30 (one tile), 1 x 1, 2 x 61 and 16 x 60 (whole tiles only); 64 -> 64 with 2 and 6 groups.  The data gradient by the direct
    kernel on the flipped bank AND by the view GEMM, each within its own bar of fp64."""
    padded_case(lib, pools, monkeypatch, s, True, ("t", "view") if s in R.DIRECT_GROUP_SHAPES or (s.B, s.H, s.W) == (2, 9, 31) else ("t",))


@pytest.mark.parametrize("s", R.DIRECT_WALK_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_direct_kernels_walk_three_tiles_per_workgroup(lib, pools, monkeypatch, s):
    """A persistent workgroup that walks at least three tiles: both input buffers are reused and the stores of a tile drain under the
    next one.  The launch arithmetic of csrc/conv.hip: LDS bytes = NS * CO * 64 (the bank; NS = 18, 9, 5 k-steps for CI = 64, 32, 16)
    + 2 * 320 * 2 CI (two input tiles with halo); slots per group = (256 CUs x 2 where two such workgroups fit into 160 KiB, else x 1)
    / groups, at most one per tile; tiles = B * ceil(H / 8) * ceil(W / 30) per group."""
    ci, co = s.C // s.groups, s.Cout // s.groups
    ty, tx = tiles(s.H, s.W)
    ntiles = s.B * ty * tx
    for CI, CO in ((ci, co), (co, ci)):                     # the forward, and the data gradient (the same kernel <co, ci> on dy)
        lds = {64: 18, 32: 9, 16: 5}[CI] * CO * 64 + 2 * 320 * 2 * CI
        slots = min(ntiles, (256 * (2 if (160 * 1024) // lds >= 2 else 1)) // s.groups)
        assert ntiles >= 3 * slots, (CI, CO, ntiles, slots)
    padded_case(lib, pools, monkeypatch, s, True, ("t",))


@pytest.mark.parametrize("s", R.VIEW_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_view_gemm_convolution(lib, pools, monkeypatch, s):
    """ci or co outside the direct pairs (asserted): the shifted views and channel groups of ia_gemm_view -- 128 -> 64, 256 -> 256,
    two groups of 8 -> 8, six 256-channel groups in one launch"""
    padded_case(lib, pools, monkeypatch, s, False, ("view",))


def test_view_gemm_data_gradient_at_a_direct_capable_shape(lib, pools, monkeypatch):
    s = R.VIEW_DGRAD_DIRECT_CAPABLE
    assert s in R.DIRECT_SHAPES       # (test_direct_kernels_at_tile_edges runs both data gradients there; this is the case by name)
    padded_case(lib, pools, monkeypatch, s, True, ("view",))


@pytest.mark.parametrize("Cin,Cout,groups", R.FLIP_SHAPES)
def test_flip_weights(lib, pools, Cin, Cout, groups):
    """every pair, and the stem's shared-input form (Cout, Cout, Cout / 64)"""
    n = Cout * 9 * (Cin // groups)
    flip(lib, pools[1]["x"][:n].view(Cout, 9 * (Cin // groups)), Cin, Cout, groups)


# ------------------------------------------------------------------------------------------------------------------ stride 2
@pytest.mark.parametrize("yc", [0, 1], ids=["bordered", "compact"])
@pytest.mark.parametrize("s", R.S2_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_stride2_kernels(lib, pools, s, yc):
    """ia_conv3x3_s2_padded_fwd / _bwd_weight / _bwd_data_t: 64 g -> 64 g with g = 1, 2, 6 and the shared-input 64 -> 128 / 192 forms, odd and
    even maps, all four parity classes of dx present and absent, output maps smaller than, equal to and one past a tile, both layouts
    of y.  The weight gradient gets dy with a NaN border (not read), the data gradient with a zero border."""
    B, H, W, Cin, Cout, g = s.B, s.H, s.W, s.C, s.Cout, s.groups
    assert lib.ia_conv3x3_s2_supported(Cin, Cout, g) == 1
    Ho, Wo = R.out_hw(s)
    n = R.shared_slices(s)
    where = "x".join(map(str, (B, H, W, Cin, Cout, g))) + (" compact" if yc else "")
    wsb = lib.ia_conv3x3_s2_padded_workspace_bytes(B, H, W, Cin, Cout, g)
    ty, tx = tiles(Ho, Wo)
    assert folds_bound(wsb, Cout, 9 * 64) >= min(B * ty * tx, 512 // (Cout // 64))
    folds = min(folds_bound(wsb, Cout, 9 * 64), B * ty * tx)        # one bank per workgroup, at most one workgroup per tile of a group
    yshape = (B, Ho, Wo, Cout) if yc else (B, Ho + 2, Wo + 2, Cout)
    lay = (lambda t, fill: t) if yc else R.to_bordered
    inner = (lambda t: t) if yc else R.interior
    for exact in (True, False):
        ops = operands(pools, s, exact)
        ref = ops["ref"]
        bar = R.bars(s, ops, "slices" if n > 1 else "gemm", L=B * ty * TH * tx * 32, folds=folds, exact=exact)
        xp, what, bias = inp(R.to_bordered(ops["x"])), inp(ops["what"]), inp(ops["bias"], F32)
        dy_nan, dy_zero = inp(lay(ops["dy"], NAN)), inp(lay(ops["dy"], 0.0))
        yp = Buf(yshape, BF16, SENT, fill=SENT)
        ok(lib.ia_conv3x3_s2_padded_fwd(xp.ptr(), what.ptr(), bias.ptr(), yp.ptr(), B, H, W, Cin, Cout, g, yc, sp()), "s2_fwd")
        torch.cuda.synchronize()
        (yp.guards_unchanged if yc else yp.border_unchanged)("s2_fwd " + where + ": yp")
        verdict("s2_padded_fwd", "y", where, inner(yp.v), ref["y"], bar["y"], exact)
        outs = []
        for _ in range(2):
            ws = workspace(wsb)
            dW = Buf((Cout, 9 * 64), F32, SENT, fill=NAN)
            db = Buf((Cout,), F32, SENT, data=ops["dbias0"])
            ok(lib.ia_conv3x3_s2_padded_bwd_weight(xp.ptr(), dy_nan.ptr(), dW.ptr(), db.ptr(), B, H, W, Cin, Cout, g, yc, ws.data_ptr(), wsb, sp()), "s2_wgrad")
            torch.cuda.synchronize()
            ws_tail_ok(ws, wsb, "s2_wgrad " + where)
            dW.guards_unchanged("s2_wgrad " + where + ": dW")
            db.guards_unchanged("s2_wgrad " + where + ": dbias")
            outs.append((dW.v.clone(), db.v.clone()))
        assert torch.equal(bits(outs[0][0]), bits(outs[1][0])) and torch.equal(bits(outs[0][1]), bits(outs[1][1])), (where, "two runs differ")
        verdict("s2_padded_bwd_weight", "dW", where, outs[0][0], ref["dW"], bar["dW"], exact)
        verdict("s2_padded_bwd_weight", "dbias", where, outs[0][1], ref["dbias"], bar["dbias"], exact)
        what_t = flip(lib, ops["what"], Cout, Cout, Cout // 64) if n > 1 else flip(lib, ops["what"], Cin, Cout, g)
        dxp = Buf((B, H + 2, W + 2, Cin), BF16, SENT, fill=SENT)
        ok(lib.ia_conv3x3_s2_padded_bwd_data_t(dy_zero.ptr(), what_t.ptr(), dxp.ptr(), B, H, W, Cin, Cout, g, yc, sp()), "s2_dgrad")
        torch.cuda.synchronize()
        dxp.border_unchanged("s2_dgrad " + where + ": dxp")
        verdict("s2_padded_bwd_data_t" + (" shared input" if n > 1 else ""), "dx", where, R.interior(dxp.v), ref["dx"], bar["dx"], exact)
        for name, b in (("xp", xp), ("what", what), ("bias", bias), ("dyp (NaN border)", dy_nan), ("dyp (zero border)", dy_zero), ("what_t", what_t)):
            b.unchanged(where + ": input " + name)
    report()


# ------------------------------------------------------------------------------------------------------------------ the patch-matrix path
def nhwc_splits(lib, s):
    Ng, K, M = s.Cout // s.groups, s.k * s.k * (s.C // s.groups), s.B * R.out_hw(s)[0] * R.out_hw(s)[1]
    b = lib.ia_gemm_workspace_bytes(Ng, K, M, 1)
    assert b % (4 * Ng * (K + 1)) == 0
    return b // (4 * Ng * (K + 1)) if b else 1


@pytest.mark.parametrize("s", R.NHWC_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_patch_matrix_path(lib, pools, s):
    """ia_conv_nhwc_fwd, _bwd_data (the dcols GEMMs and the gather-form col2im3_kernel) and _bwd_weight at small shapes: stride 1 and 2,
    groups 1, 2 and 6 (Cg = 8, the smallest), a 1 x 1 map, 256 -> 512, and the k = 1 form.  cols_valid = 1 after a forward on the same
    workspace equals cols_valid = 0; dbias = NULL leaves dW as it is with one."""
    B, H, W, C, Cout, k, st, g = s
    Ho, Wo = R.out_hw(s)
    M, K = B * Ho * Wo, k * k * (C // g)
    where = "x".join(map(str, s))
    wsb = lib.ia_conv_nhwc_workspace_bytes(B, H, W, C, Cout, k, st, g)
    splits = nhwc_splits(lib, s)
    for exact in (True, False):
        ops = operands(pools, s, exact, cols=True)
        ref = ops["ref"]
        bar = R.bars(s, ops, "cols" if k == 3 else "gemm", L=M, folds=splits, exact=exact)
        x, dy, what, bias = inp(ops["x"]), inp(ops["dy"]), inp(ops["what"]), inp(ops["bias"], F32)
        ws = workspace(wsb)
        wp = ws.data_ptr()
        y = Buf((B, Ho, Wo, Cout), BF16, SENT, fill=SENT)
        ok(lib.ia_conv_nhwc_fwd(x.ptr(), what.ptr(), bias.ptr(), y.ptr(), B, H, W, C, Cout, k, st, g, wp, wsb, sp()), "nhwc_fwd")
        torch.cuda.synchronize()
        y.guards_unchanged("nhwc_fwd " + where + ": y")
        verdict("conv_nhwc_fwd k=%d" % k, "y", where, y.v, ref["y"], bar["y"], exact)

        def wgrad(cols_valid, with_bias):
            dW = Buf((Cout, K), F32, SENT, fill=NAN)
            db = Buf((Cout,), F32, SENT, data=ops["dbias0"])
            ok(lib.ia_conv_nhwc_bwd_weight(x.ptr(), dy.ptr(), dW.ptr(), db.ptr() if with_bias else None, B, H, W, C, Cout, k, st, g, cols_valid, wp, wsb,
                                           sp()), "nhwc_wgrad")
            torch.cuda.synchronize()
            dW.guards_unchanged("nhwc_wgrad " + where + ": dW")
            (db.guards_unchanged if with_bias else db.unchanged)("nhwc_wgrad " + where + ": dbias")
            return dW.v.clone(), db.v.clone()

        reused = wgrad(1, True)                       # (the forward above left its patch matrix in the workspace)
        ws.fill_(0x5A)
        fresh = wgrad(0, True)
        assert torch.equal(bits(fresh[0]), bits(reused[0])) and torch.equal(bits(fresh[1]), bits(reused[1])), (where, "cols_valid = 1 differs from 0")
        nobias = wgrad(0, False)
        assert torch.equal(bits(fresh[0]), bits(nobias[0])), (where, "dW depends on dbias being there")
        verdict("conv_nhwc_bwd_weight k=%d" % k, "dW", where, fresh[0], ref["dW"], bar["dW"], exact)
        verdict("conv_nhwc_bwd_weight k=%d" % k, "dbias", where, fresh[1], ref["dbias"], bar["dbias"], exact)
        dx = Buf((B, H, W, C), BF16, SENT, fill=SENT)
        ok(lib.ia_conv_nhwc_bwd_data(dy.ptr(), what.ptr(), dx.ptr(), B, H, W, C, Cout, k, st, g, wp, wsb, sp()), "nhwc_dgrad")
        torch.cuda.synchronize()
        dx.guards_unchanged("nhwc_dgrad " + where + ": dx")
        verdict("conv_nhwc_bwd_data k=%d" % k, "dx", where, dx.v, ref["dx"], bar["dx"], exact)
        ws_tail_ok(ws, wsb, where)
        for name, b in (("x", x), ("dy", dy), ("what", what), ("bias", bias)):
            b.unchanged(where + ": input " + name)
    report()


@pytest.mark.parametrize("why,shape,code", [("k = 2", (2, 7, 9, 64, 64, 2, 1, 1), IA_ERR_ARG), ("stride 3", (2, 7, 9, 64, 64, 3, 3, 1), IA_ERR_ARG),
                                            ("k = 1 with stride 2", (2, 7, 9, 64, 64, 1, 2, 1), IA_ERR_UNSUPPORTED),
                                            ("k = 1 with groups 2", (2, 7, 9, 64, 64, 1, 1, 2), IA_ERR_UNSUPPORTED),
                                            ("Cg no multiple of 8", (2, 7, 9, 24, 48, 3, 1, 2), IA_ERR_ARG),
                                            ("the workspace one byte short", (2, 7, 9, 64, 64, 3, 1, 1), IA_ERR_WORKSPACE)])
def test_patch_matrix_path_refusals(lib, why, shape, code):
    """geom's refusals and the workspace check come back before any launch: the documented code, every output still the sentinel.  All
    pointers are real buffers large enough for the nearest legal shape, so nothing that a wrong launch could touch is unmapped."""
    B, H, W, C, Cout, k, st, g = shape
    n = 1 << 20
    x, dy, what = (Buf((n,), BF16, NAN, fill=1.0) for _ in range(3))
    y, dx = Buf((n,), BF16, SENT, fill=SENT), Buf((n,), BF16, SENT, fill=SENT)
    dW, db = Buf((n,), F32, SENT, fill=SENT), Buf((4096,), F32, SENT, fill=SENT)
    short = code == IA_ERR_WORKSPACE
    wsb = lib.ia_conv_nhwc_workspace_bytes(B, H, W, C, Cout, k, st, g)
    assert (wsb > 0) == short, (why, "the workspace query answers 0 for a shape that is refused")
    ws = workspace(4 << 20)
    given = wsb - 1 if short else 4 << 20
    assert lib.ia_conv_nhwc_fwd(x.ptr(), what.ptr(), None, y.ptr(), B, H, W, C, Cout, k, st, g, ws.data_ptr(), given, sp()) == code, why
    assert lib.ia_conv_nhwc_bwd_data(dy.ptr(), what.ptr(), dx.ptr(), B, H, W, C, Cout, k, st, g, ws.data_ptr(), given, sp()) == code, why
    assert lib.ia_conv_nhwc_bwd_weight(x.ptr(), dy.ptr(), dW.ptr(), db.ptr(), B, H, W, C, Cout, k, st, g, 0, ws.data_ptr(), given, sp()) == code, why
    torch.cuda.synchronize()
    for name, b in (("y", y), ("dx", dx), ("dW", dW), ("dbias", db), ("x", x), ("dy", dy), ("what", what)):
        b.unchanged(why + ": " + name)
    assert bool((ws == 0x5A).all()), why + ": the workspace was written"
