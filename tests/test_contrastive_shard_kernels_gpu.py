"""ia_contrastive_shard_fwd / ia_contrastive_shard_bwd through the C ABI against the fp64 reference of
tests/contrastive_shard_reference.py computed from the same fp32 inputs, element by element.  The bars are derived there from the
summation chains csrc/contrastive.hip states and the 1 ulp of expf / logf, not measured.  Every helper prints the largest error it saw
as a fraction of its bound (`-s` shows them); that figure is recorded, never used to set a bound.

Beyond the bounds: at world = 1 the shard entries are bit for bit the square entries; two runs agree bit for bit; dlog_scale accumulates;
argument errors touch nothing; the ops wrappers are the C ABI; and shards of one batch run one after another assemble to the fp64
result of the whole batch (the invariant of the data-parallel step, on one GPU and without a process group).
"""
import pytest
import torch

import contrastive_reference as R
import contrastive_shard_reference as S

pytestmark = pytest.mark.gpu

F64, F32 = torch.float64, torch.float32
DLOSS = 0.75
CANARY = 123.0


@pytest.fixture(scope="module")
def lib(gpu):
    from item_alignment_amd import _lib
    return _lib.load()


def st():
    from item_alignment_amd import _lib
    return _lib.stream_ptr()


def padded(x, ld, fill):
    out = torch.full((x.shape[0], ld), fill, dtype=F32)
    out[:, :x.shape[1]] = x
    return out


def square_forward(lib, t, im, log_scale):
    """ia_contrastive_fwd on the whole batch -> the device tensors loss, sim, lse_row, lse_col (what every rank would hold of the
    gathered log-sum-exps)"""
    from item_alignment_amd import _lib
    G, H = t.shape
    td, imd, ls = t.cuda(), im.cuda(), torch.tensor([log_scale], dtype=F32, device="cuda")
    sim, lse_row, lse_col, loss = (torch.empty(s, device="cuda") for s in ((G, G), (G,), (G,), (1,)))
    ws_bytes = lib.ia_contrastive_workspace_bytes(G)
    ws = torch.empty(ws_bytes, device="cuda", dtype=torch.uint8)
    _lib.check(lib.ia_contrastive_fwd(td.data_ptr(), H, imd.data_ptr(), H, ls.data_ptr(), sim.data_ptr(), G, lse_row.data_ptr(),
                                      lse_col.data_ptr(), loss.data_ptr(), G, H, ws.data_ptr(), ws_bytes, st()), "ia_contrastive_fwd")
    return dict(loss=loss, sim=sim, lse_row=lse_row, lse_col=lse_col, ws=ws, ws_bytes=ws_bytes, text=td, image=imd, ls=ls)


def run(lib, t, im, log_scale, o, B, world, pads=(0,) * 7, dloss=DLOSS, preset=None, lse_g=None):
    """One shard forward + backward: rows o .. o + B - 1 of the gathered t, im [G, H].  pads: extra columns of text_l, image_l, text_g,
    image_g, sim_t / sim_i, dtext_l, dimage_l; the input pads hold NaN, the output pads a canary.  lse_g: (lse_row_g, lse_col_g) device
    tensors for the backward (default: the square kernel's on the whole batch).  preset: dlog_scale starts at that value and the call
    accumulates.  -> dict of device tensors, padded as they were passed."""
    from item_alignment_amd import _lib
    G, H = t.shape
    ldtl, ldil, ldtg, ldig, lds, lddt, lddi = (n + p for n, p in zip((H, H, H, H, G, H, H), pads))
    nan = float("nan")
    tl, il = padded(t[o:o + B], ldtl, nan).cuda(), padded(im[o:o + B], ldil, nan).cuda()
    tg, ig = padded(t, ldtg, nan).cuda(), padded(im, ldig, nan).cuda()
    ls = torch.tensor([log_scale], dtype=F32, device="cuda")
    sim_t, sim_i = torch.full((B, lds), CANARY, device="cuda"), torch.full((B, lds), CANARY, device="cuda")
    lse_row_l, lse_col_l = torch.full((B,), CANARY, device="cuda"), torch.full((B,), CANARY, device="cuda")
    loss = torch.full((1,), CANARY, device="cuda")
    ws_bytes = lib.ia_contrastive_shard_workspace_bytes(B, G)
    assert ws_bytes >= (2 * B * G + B) * 4
    ws = torch.full((ws_bytes,), 0xFF, device="cuda", dtype=torch.uint8)       # NaN bit patterns: nothing may depend on what it held
    _lib.check(lib.ia_contrastive_shard_fwd(tl.data_ptr(), ldtl, il.data_ptr(), ldil, tg.data_ptr(), ldtg, ig.data_ptr(), ldig, ls.data_ptr(),
                                            sim_t.data_ptr(), sim_i.data_ptr(), lds, lse_row_l.data_ptr(), lse_col_l.data_ptr(),
                                            loss.data_ptr(), B, G, o, world, H, ws.data_ptr(), ws_bytes, st()), "ia_contrastive_shard_fwd")
    if lse_g is None:
        sq = square_forward(lib, t, im, log_scale)
        lse_g = (sq["lse_row"], sq["lse_col"])
    ws.fill_(0xFF)
    dl = torch.tensor([dloss], dtype=F32, device="cuda")
    dtext, dimage = torch.full((B, lddt), CANARY, device="cuda"), torch.full((B, lddi), CANARY, device="cuda")
    dls = torch.tensor([CANARY if preset is None else preset], dtype=F32, device="cuda")
    _lib.check(lib.ia_contrastive_shard_bwd(tg.data_ptr(), ldtg, ig.data_ptr(), ldig, ls.data_ptr(), sim_t.data_ptr(), sim_i.data_ptr(), lds,
                                            lse_g[0].data_ptr(), lse_g[1].data_ptr(), dl.data_ptr(), dtext.data_ptr(), lddt,
                                            dimage.data_ptr(), lddi, dls.data_ptr(), int(preset is not None), B, G, o, world, H,
                                            ws.data_ptr(), ws_bytes, st()), "ia_contrastive_shard_bwd")
    torch.cuda.synchronize()
    return dict(sim_t=sim_t, sim_i=sim_i, lse_row_l=lse_row_l, lse_col_l=lse_col_l, loss=loss, dtext_l=dtext, dimage_l=dimage,
                dlog_scale=dls)


def close(name, got, want, bound):
    got, want, bound = got.detach().cpu().to(F64).reshape(-1), want.to(F64).reshape(-1), bound.to(F64).reshape(-1)
    err = (got - want).abs()
    assert torch.isfinite(got).all(), (name, "non-finite output")
    r = float((err / bound).max())
    print(f"[contrastive shard] {name}: max error / bound = {r:.3f}")
    assert r <= 1.0, (name, r)
    return r


def check_case(lib, t, im, log_scale, o, B, world, tag, pads=(0,) * 7, preset=None):
    G, H = t.shape
    out = run(lib, t, im, log_scale, o, B, world, pads=pads, preset=preset)
    ls32 = float(torch.tensor(log_scale, dtype=F32))
    glob = R.forward(t, im, ls32)
    f = S.forward(t, im, ls32, o, B, world)
    b = S.backward(t, im, ls32, o, B, world, dloss=DLOSS, fwd=f, glob=glob, accumulated_onto=0.0 if preset is None else preset)
    close(f"{tag} sim_t (c = {R.dot_chain(H) + 1})", out["sim_t"][:, :G], f["sim_t"], f["sim_t_bound"])
    close(f"{tag} sim_i", out["sim_i"][:, :G], f["sim_i"], f["sim_i_bound"])
    close(f"{tag} lse_row_l (c = {R.wave_chain(G)})", out["lse_row_l"], f["lse_row_l"], f["lse_row_l_bound"])
    close(f"{tag} lse_col_l", out["lse_col_l"], f["lse_col_l"], f["lse_col_l_bound"])
    close(f"{tag} loss", out["loss"], f["loss"], f["loss_bound"])
    close(f"{tag} dtext_l (c = {R.dot_chain(G) + 1})", out["dtext_l"][:, :H], b["dtext_l"], b["dtext_l_bound"])
    close(f"{tag} dimage_l", out["dimage_l"][:, :H], b["dimage_l"], b["dimage_l_bound"])
    close(f"{tag} dlog_scale", out["dlog_scale"], b["dlog_scale"], b["dlog_scale_bound"])
    for name, width in (("sim_t", G), ("sim_i", G), ("dtext_l", H), ("dimage_l", H)):
        assert (out[name][:, width:] == CANARY).all(), (name, "a pad column was written")
    return out, f, b


@pytest.fixture(scope="module")
def inputs():
    """every (G, H, kind) gathered batch once, on the host"""
    return {(G, H, kind): R.build(G, H, kind, seed=1000 + 7 * G + H + R.KINDS.index(kind))
            for G, H in sorted({(s[1], s[3]) for s in S.SHAPES} | {(3, 128), (65, 768), (257, 128), (65, 192)}) for kind in R.KINDS}


def pads_of(B, G):
    return (5, 3, 4, 6, 2, 1, 7) if (B, G) in ((3, 7), (17, 65), (3, 3)) else (0,) * 7


@pytest.mark.parametrize("kind", R.KINDS)
@pytest.mark.parametrize("B,G,o,H", S.SHAPES)
def test_forward_and_backward_against_fp64(lib, inputs, B, G, o, H, kind):
    t, im = inputs[(G, H, kind)]
    for log_scale in R.LOG_SCALES:
        check_case(lib, t, im, log_scale, o, B, S.world_of(B, G), f"{B}/{G}@{o}x{H} {kind} ls={log_scale}", pads=pads_of(B, G))


@pytest.mark.parametrize("B,H", [(3, 128), (65, 768), (257, 128)])
def test_world_one_is_bit_identical_to_the_square_kernels(lib, inputs, B, H):
    """the cheapest proof that the shard path computes the old function: same chains, so the same bits"""
    from item_alignment_amd import _lib
    t, im = inputs[(B, H, "random")]
    for log_scale in (1.0, 4.6):
        sq = square_forward(lib, t, im, log_scale)
        dl = torch.tensor([DLOSS], dtype=F32, device="cuda")
        dtext, dimage, dls = torch.empty(B, H, device="cuda"), torch.empty(B, H, device="cuda"), torch.empty(1, device="cuda")
        _lib.check(lib.ia_contrastive_bwd(sq["text"].data_ptr(), H, sq["image"].data_ptr(), H, sq["ls"].data_ptr(), sq["sim"].data_ptr(), B,
                                          sq["lse_row"].data_ptr(), sq["lse_col"].data_ptr(), dl.data_ptr(), dtext.data_ptr(), H,
                                          dimage.data_ptr(), H, dls.data_ptr(), 0, B, H, sq["ws"].data_ptr(), sq["ws_bytes"], st()),
                   "ia_contrastive_bwd")
        got = run(lib, t, im, log_scale, 0, B, 1, pads=pads_of(B, B), lse_g=(sq["lse_row"], sq["lse_col"]))
        torch.cuda.synchronize()
        bits = lambda x: x.contiguous().view(torch.int32)
        for name, a, b in (("sim_t", got["sim_t"][:, :B], sq["sim"]), ("sim_i", got["sim_i"][:, :B], sq["sim"].T),
                           ("lse_row_l", got["lse_row_l"], sq["lse_row"]), ("lse_col_l", got["lse_col_l"], sq["lse_col"]),
                           ("loss", got["loss"], sq["loss"]), ("dtext_l", got["dtext_l"][:, :H], dtext),
                           ("dimage_l", got["dimage_l"][:, :H], dimage), ("dlog_scale", got["dlog_scale"], dls)):
            assert torch.equal(bits(a), bits(b)), (name, log_scale)


@pytest.mark.parametrize("B,G,o,H", [(3, 7, 4, 128), (17, 65, 48, 192), (16, 257, 100, 128)])
def test_two_runs_are_bit_identical(lib, inputs, B, G, o, H):
    t, im = inputs[(G, H, "random")]
    a, b = (run(lib, t, im, 1.0, o, B, S.world_of(B, G), pads=pads_of(B, G)) for _ in range(2))
    for name in a:
        assert torch.equal(a[name].view(torch.int32), b[name].view(torch.int32)), name


@pytest.mark.parametrize("B,G,o,H", [(3, 7, 4, 128), (64, 128, 64, 768)])
def test_dlog_scale_accumulates_onto_a_preset_value(lib, inputs, B, G, o, H):
    t, im = inputs[(G, H, "random")]
    W = S.world_of(B, G)
    fresh, _, _ = check_case(lib, t, im, 1.0, o, B, W, f"{B}/{G} fresh", pads=pads_of(B, G))
    added, _, _ = check_case(lib, t, im, 1.0, o, B, W, f"{B}/{G} accumulate", pads=pads_of(B, G), preset=2.5)
    assert float(added["dlog_scale"]) == float(torch.tensor(2.5, dtype=F32) + fresh["dlog_scale"].cpu()[0])


def test_argument_checks_leave_the_outputs_alone(lib):
    """every refusal comes before a launch: the outputs keep what they held"""
    B, G, o, H = 4, 10, 3, 16
    tg, ig = torch.randn(G, H, device="cuda"), torch.randn(G, H, device="cuda")
    tl, il = tg[o:o + B].contiguous(), ig[o:o + B].contiguous()
    ls, dl = torch.zeros(1, device="cuda"), torch.ones(1, device="cuda")
    sizes = [B * G, B * G, B, B, 1, B * H, B * H, 1]
    out = torch.full((sum(sizes),), 7.0, device="cuda")
    st_, si_, lr, lc, lo, dt, di, dls = torch.split(out, sizes)
    lrg, lcg = torch.zeros(G, device="cuda"), torch.zeros(G, device="cuda")
    ws_bytes = lib.ia_contrastive_shard_workspace_bytes(B, G)
    assert lib.ia_contrastive_shard_workspace_bytes(0, G) == 0 and lib.ia_contrastive_shard_workspace_bytes(B, 0) == 0
    ws = torch.empty(ws_bytes, device="cuda", dtype=torch.uint8)
    TL, IL, TG, IG, LS, ST, SI, LR, LC, LO, DL, DT, DI, DLS, LRG, LCG, W = (
        x.data_ptr() for x in (tl, il, tg, ig, ls, st_, si_, lr, lc, lo, dl, dt, di, dls, lrg, lcg, ws))

    def fwd(tl=TL, ldtl=H, ldil=H, tg=TG, ldtg=H, ldig=H, si=SI, lds=G, lo=LO, b=B, g=G, o=o, world=2, h=H, w=W, wb=ws_bytes):
        return lib.ia_contrastive_shard_fwd(tl, ldtl, IL, ldil, tg, ldtg, IG, ldig, LS, ST, si, lds, LR, LC, lo, b, g, o, world, h, w, wb, st())

    def bwd(tg=TG, ldtg=H, ldig=H, lds=G, lrg=LRG, lddt=H, lddi=H, dls=DLS, b=B, g=G, o=o, world=2, h=H, w=W, wb=ws_bytes):
        return lib.ia_contrastive_shard_bwd(tg, ldtg, IG, ldig, LS, ST, SI, lds, lrg, LCG, DL, DT, lddt, DI, lddi, dls, 0, b, g, o, world, h,
                                            w, wb, st())

    for kw in (dict(tl=None), dict(tg=None), dict(si=None), dict(lo=None), dict(ldtl=H - 1), dict(ldil=H - 1), dict(ldtg=H - 1),
               dict(ldig=H - 1), dict(lds=G - 1), dict(b=0), dict(b=-1), dict(g=0), dict(h=0), dict(o=-1), dict(o=G - B + 1), dict(b=G + 1, o=0),
               dict(world=0), dict(o=2 ** 31 - 2)):
        assert fwd(**kw) == -1, kw
    for kw in (dict(tg=None), dict(lrg=None), dict(dls=None), dict(ldtg=H - 1), dict(ldig=H - 1), dict(lds=G - 1), dict(lddt=H - 1),
               dict(lddi=H - 1), dict(b=0), dict(g=0), dict(h=0), dict(o=-1), dict(o=G - B + 1), dict(world=0), dict(o=2 ** 31 - 2)):
        assert bwd(**kw) == -1, kw
    assert fwd(w=None) == -3 and fwd(wb=ws_bytes - 1) == -3 and bwd(w=None) == -3 and bwd(wb=ws_bytes - 1) == -3
    torch.cuda.synchronize()
    assert (out == 7.0).all()
    assert fwd() == 0
    lrg.fill_(1.0); lcg.fill_(1.0)
    assert bwd() == 0
    torch.cuda.synchronize()
    assert torch.isfinite(out).all() and not (out == 7.0).any()


def test_ops_wrappers_agree_with_the_c_abi(lib, inputs):
    """ops.contrastive_shard_fwd / contrastive_shard_bwd give bit for bit what the direct calls give"""
    from item_alignment_amd import ops
    B, G, o, H, W = 17, 65, 48, 192, 4
    t, im = inputs[(G, H, "random")]
    want = run(lib, t, im, 1.0, o, B, W)
    sq = square_forward(lib, t, im, 1.0)
    ls, dl = torch.tensor([1.0], device="cuda"), torch.tensor([DLOSS], device="cuda")
    tg, ig = t.cuda(), im.cuda()
    loss, sim_t, sim_i, lse_row_l, lse_col_l = ops.contrastive_shard_fwd(tg[o:o + B].contiguous(), ig[o:o + B].contiguous(), tg, ig, ls, o, W)
    dtext, dimage, dls = ops.contrastive_shard_bwd(tg, ig, ls, sim_t, sim_i, sq["lse_row"], sq["lse_col"], dl, o, W)
    for name, got in (("loss", loss), ("sim_t", sim_t), ("sim_i", sim_i), ("lse_row_l", lse_row_l), ("lse_col_l", lse_col_l),
                      ("dtext_l", dtext), ("dimage_l", dimage), ("dlog_scale", dls)):
        assert torch.equal(got, want[name]), name
    preset = torch.tensor([2.5], device="cuda")
    ops.contrastive_shard_bwd(tg, ig, ls, sim_t, sim_i, sq["lse_row"], sq["lse_col"], dl, o, W, dlog_scale=preset, accumulate=True)
    assert float(preset) == float(torch.tensor(2.5) + dls.cpu()[0])


@pytest.mark.parametrize("split", [(17, 48), (3, 17, 45)], ids=lambda s: "+".join(map(str, s)))
def test_shards_run_one_after_another_assemble_to_the_whole_batch(lib, inputs, split):
    """What the ranks of a data-parallel step do, on one GPU: every shard's forward, the log-sum-exps concatenated rank-major, every
    shard's backward.  The mean loss, the stacked gradients / world and the summed dlog_scale / world are held to the fp64 result of the
    whole batch, within its bounds plus what the shard reference adds for den and the shorter sums (both from the references)."""
    G, W, H = sum(split), len(split), 192
    t, im = inputs[(G, H, "random")]
    ls32 = float(torch.tensor(1.0, dtype=F32))
    glob = R.forward(t, im, ls32)
    gb = R.backward(t, im, ls32, dloss=DLOSS, fwd=glob)
    offs = [sum(split[:r]) for r in range(W)]
    fwds = [run(lib, t, im, 1.0, o, B, W) for o, B in zip(offs, split)]
    lse_g = (torch.cat([f["lse_row_l"] for f in fwds]), torch.cat([f["lse_col_l"] for f in fwds]))
    close("gathered lse_row", lse_g[0], glob["lse_row"], glob["lse_row_bound"])
    close("gathered lse_col", lse_g[1], glob["lse_col"], glob["lse_col_bound"])
    outs = [run(lib, t, im, 1.0, o, B, W, lse_g=lse_g) for o, B in zip(offs, split)]
    refs = [S.backward(t, im, ls32, o, B, W, dloss=DLOSS, glob=glob) for o, B in zip(offs, split)]
    fref = [S.forward(t, im, ls32, o, B, W) for o, B in zip(offs, split)]
    # the mean of W shard losses: each within its own bound, one more rounding for the mean
    loss = torch.stack([x["loss"].cpu().to(F64)[0] for x in outs]).mean()
    loss_bound = torch.stack([f["loss_bound"] for f in fref]).mean() + R.U24 * glob["loss"].abs()
    close("mean loss", loss, glob["loss"], loss_bound)
    for name, key in (("dtext_l", "dtext"), ("dimage_l", "dimage")):
        got = torch.cat([x[name] for x in outs]).cpu().to(F64) / W
        bound = torch.cat([r[name + "_bound"] for r in refs]) / W + R.U24 * gb[key].abs()
        close(f"stacked {name} / world", got, gb[key], bound)
    dls = sum(float(x["dlog_scale"]) for x in outs) / W
    dls_bound = sum(float(r["dlog_scale_bound"]) for r in refs) / W + R.U24 * abs(float(gb["dlog_scale"]))
    close("summed dlog_scale / world", torch.tensor(dls, dtype=F64), gb["dlog_scale"], torch.tensor(dls_bound, dtype=F64))
