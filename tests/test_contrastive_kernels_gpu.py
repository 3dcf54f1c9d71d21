"""ia_contrastive_fwd / ia_contrastive_bwd through the C ABI against the fp64 reference of tests/contrastive_reference.py computed from
the same fp32 inputs, element by element.  The bars are derived there from the summation chains csrc/contrastive.hip states and the
1 ulp of expf / logf, not measured: |got - want| <= the reference's bound for sim, lse_row, lse_col, the loss, dtext, dimage and
dlog_scale.  Every helper prints the largest error it saw as a fraction of its bound (`-s` shows them); that figure is recorded, never
used to set a bound.
"""
import math

import pytest
import torch

import contrastive_reference as R

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


def run(lib, t, im, log_scale, pads=(0, 0, 0, 0, 0), dloss=DLOSS, preset=None):
    """One forward + backward.  pads: extra columns of text, image, sim, dtext, dimage; the input pads hold NaN, the output pads a canary.
    preset: dlog_scale starts at that value and the call accumulates.  -> dict of device tensors, padded as they were passed."""
    from item_alignment_amd import _lib
    B, H = t.shape
    ldt, ldi, lds, lddt, lddi = H + pads[0], H + pads[1], B + pads[2], H + pads[3], H + pads[4]
    td, imd = padded(t, ldt, float("nan")).cuda(), padded(im, ldi, float("nan")).cuda()
    ls = torch.tensor([log_scale], dtype=F32, device="cuda")
    sim = torch.full((B, lds), CANARY, device="cuda")
    lse_row, lse_col = torch.full((B,), CANARY, device="cuda"), torch.full((B,), CANARY, device="cuda")
    loss = torch.full((1,), CANARY, device="cuda")
    ws_bytes = lib.ia_contrastive_workspace_bytes(B)
    ws = torch.full((ws_bytes,), 0xFF, device="cuda", dtype=torch.uint8)       # NaN bit patterns: nothing may depend on what it held
    _lib.check(lib.ia_contrastive_fwd(td.data_ptr(), ldt, imd.data_ptr(), ldi, ls.data_ptr(), sim.data_ptr(), lds, lse_row.data_ptr(),
                                      lse_col.data_ptr(), loss.data_ptr(), B, H, ws.data_ptr(), ws_bytes, st()), "ia_contrastive_fwd")
    ws.fill_(0xFF)
    dl = torch.tensor([dloss], dtype=F32, device="cuda")
    dtext, dimage = torch.full((B, lddt), CANARY, device="cuda"), torch.full((B, lddi), CANARY, device="cuda")
    dls = torch.tensor([CANARY if preset is None else preset], dtype=F32, device="cuda")
    _lib.check(lib.ia_contrastive_bwd(td.data_ptr(), ldt, imd.data_ptr(), ldi, ls.data_ptr(), sim.data_ptr(), lds, lse_row.data_ptr(),
                                      lse_col.data_ptr(), dl.data_ptr(), dtext.data_ptr(), lddt, dimage.data_ptr(), lddi, dls.data_ptr(),
                                      int(preset is not None), B, H, ws.data_ptr(), ws_bytes, st()), "ia_contrastive_bwd")
    torch.cuda.synchronize()
    return dict(sim=sim, lse_row=lse_row, lse_col=lse_col, loss=loss, dtext=dtext, dimage=dimage, dlog_scale=dls)


def close(name, got, want, bound):
    got, want, bound = got.detach().cpu().to(F64).reshape(-1), want.to(F64).reshape(-1), bound.to(F64).reshape(-1)
    err = (got - want).abs()
    assert torch.isfinite(got).all(), (name, "non-finite output")
    r = float((err / bound).max())
    print(f"[contrastive] {name}: max error / bound = {r:.3f}")
    assert r <= 1.0, (name, r)
    return r


def check_case(lib, t, im, log_scale, tag, pads=(0, 0, 0, 0, 0), preset=None):
    B, H = t.shape
    out = run(lib, t, im, log_scale, pads=pads, preset=preset)
    ls32 = float(torch.tensor(log_scale, dtype=F32))
    f = R.forward(t, im, ls32)
    b = R.backward(t, im, ls32, dloss=DLOSS, fwd=f, accumulated_onto=0.0 if preset is None else preset)
    close(f"{tag} sim (c = {R.dot_chain(H) + 1})", out["sim"][:, :B], f["sim"], f["sim_bound"])
    close(f"{tag} lse_row (c = {R.wave_chain(B)})", out["lse_row"], f["lse_row"], f["lse_row_bound"])
    close(f"{tag} lse_col", out["lse_col"], f["lse_col"], f["lse_col_bound"])
    close(f"{tag} loss", out["loss"], f["loss"], f["loss_bound"])
    close(f"{tag} dtext (c = {R.dot_chain(B) + 1})", out["dtext"][:, :H], b["dtext"], b["dtext_bound"])
    close(f"{tag} dimage", out["dimage"][:, :H], b["dimage"], b["dimage_bound"])
    close(f"{tag} dlog_scale", out["dlog_scale"], b["dlog_scale"], b["dlog_scale_bound"])
    for name, width in (("sim", B), ("dtext", H), ("dimage", H)):
        assert (out[name][:, width:] == CANARY).all(), (name, "a pad column was written")
    return out, f, b


@pytest.fixture(scope="module")
def inputs():
    """every (shape, kind) input once, on the host"""
    return {(B, H, kind): R.build(B, H, kind, seed=1000 + 7 * B + H + R.KINDS.index(kind)) for B, H in R.SHAPES for kind in R.KINDS}


def pads_of(B, H):
    return (5, 3, 2, 1, 7) if (B, H) == (3, 128) else (0, 0, 0, 0, 0)


@pytest.mark.parametrize("kind", R.KINDS)
@pytest.mark.parametrize("B,H", R.SHAPES)
def test_forward_and_backward_against_fp64(lib, inputs, B, H, kind):
    t, im = inputs[(B, H, kind)]
    for log_scale in R.LOG_SCALES:
        out, f, b = check_case(lib, t, im, log_scale, f"{B}x{H} {kind} ls={log_scale}", pads=pads_of(B, H))
        if kind == "equal":
            assert abs(float(out["loss"]) - math.log(B)) <= float(f["loss_bound"])
        if B == 1:
            for name, bound in (("loss", f["loss_bound"]), ("dtext", b["dtext_bound"]), ("dimage", b["dimage_bound"]),
                                ("dlog_scale", b["dlog_scale_bound"])):
                width = H if name in ("dtext", "dimage") else 1
                assert (out[name].cpu().to(F64).reshape(1, -1)[:, :width].abs() <= bound.reshape(1, -1)).all(), name


@pytest.mark.parametrize("B,H", [(3, 128), (65, 768), (257, 128)])
def test_two_runs_are_bit_identical(lib, inputs, B, H):
    t, im = inputs[(B, H, "random")]
    a, b = run(lib, t, im, 1.0, pads=pads_of(B, H)), run(lib, t, im, 1.0, pads=pads_of(B, H))
    for name in a:
        assert torch.equal(a[name].view(torch.int32), b[name].view(torch.int32)), name


@pytest.mark.parametrize("B,H", [(3, 128), (64, 768)])
def test_dlog_scale_accumulates_onto_a_preset_value(lib, inputs, B, H):
    t, im = inputs[(B, H, "random")]
    fresh, _, _ = check_case(lib, t, im, 1.0, f"{B}x{H} fresh", pads=pads_of(B, H))
    added, _, _ = check_case(lib, t, im, 1.0, f"{B}x{H} accumulate", pads=pads_of(B, H), preset=2.5)
    assert float(added["dlog_scale"]) == float(torch.tensor(2.5, dtype=F32) + fresh["dlog_scale"].cpu()[0])


def test_argument_checks_leave_the_outputs_alone(lib):
    """every refusal comes before a launch: the outputs keep what they held"""
    B, H = 4, 16
    t, im = torch.randn(B, H, device="cuda"), torch.randn(B, H, device="cuda")
    ls, dl = torch.zeros(1, device="cuda"), torch.ones(1, device="cuda")
    out = torch.full((B * B + 2 * B + 1 + 2 * B * H + 1,), 7.0, device="cuda")
    sim, lr, lc, lo = out[:B * B], out[B * B:B * B + B], out[B * B + B:B * B + 2 * B], out[B * B + 2 * B:B * B + 2 * B + 1]
    o = B * B + 2 * B + 1
    dt, di, dls = out[o:o + B * H], out[o + B * H:o + 2 * B * H], out[o + 2 * B * H:]
    ws_bytes = lib.ia_contrastive_workspace_bytes(B)
    ws = torch.empty(ws_bytes, device="cuda", dtype=torch.uint8)
    T, I, LS, S, LR, LC, LO, DL, DT, DI, DLS, W = (x.data_ptr() for x in (t, im, ls, sim, lr, lc, lo, dl, dt, di, dls, ws))

    def fwd(t=T, ldt=H, lds=B, b=B, h=H, w=W, wb=ws_bytes, lo=LO):
        return lib.ia_contrastive_fwd(t, ldt, I, H, LS, S, lds, LR, LC, lo, b, h, w, wb, st())

    def bwd(t=T, lddt=H, lddi=H, b=B, h=H, w=W, wb=ws_bytes, dls=DLS):
        return lib.ia_contrastive_bwd(t, H, I, H, LS, S, B, LR, LC, DL, DT, lddt, DI, lddi, dls, 0, b, h, w, wb, st())

    for kw in (dict(t=None), dict(lo=None), dict(ldt=H - 1), dict(lds=B - 1), dict(b=0), dict(h=0)):
        assert fwd(**kw) == -1, kw
    for kw in (dict(t=None), dict(dls=None), dict(lddt=H - 1), dict(lddi=H - 1), dict(b=0), dict(h=0)):
        assert bwd(**kw) == -1, kw
    assert fwd(w=None) == -3 and fwd(wb=ws_bytes - 1) == -3 and bwd(w=None) == -3 and bwd(wb=ws_bytes - 1) == -3
    torch.cuda.synchronize()
    assert (out == 7.0).all()
    assert fwd() == 0 and bwd() == 0
    torch.cuda.synchronize()
    assert torch.isfinite(out).all() and not (out == 7.0).any()


def test_ops_wrappers_agree_with_the_c_abi(lib, inputs):
    """ops.contrastive_fwd / contrastive_bwd give bit for bit what the direct calls give"""
    from item_alignment_amd import ops
    t, im = inputs[(17, 192, "random")]
    want = run(lib, t, im, 1.0)
    ls, dl = torch.tensor([1.0], device="cuda"), torch.tensor([DLOSS], device="cuda")
    loss, sim, lse_row, lse_col = ops.contrastive_fwd(t.cuda(), im.cuda(), ls)
    dtext, dimage, dls = ops.contrastive_bwd(t.cuda(), im.cuda(), ls, sim, lse_row, lse_col, dl)
    for name, got in (("loss", loss), ("sim", sim), ("lse_row", lse_row), ("lse_col", lse_col), ("dtext", dtext), ("dimage", dimage),
                      ("dlog_scale", dls)):
        assert torch.equal(got, want[name]), name
    preset = torch.tensor([2.5], device="cuda")
    ops.contrastive_bwd(t.cuda(), im.cuda(), ls, sim, lse_row, lse_col, dl, dlog_scale=preset, accumulate=True)
    assert float(preset) == float(torch.tensor(2.5) + dls.cpu()[0])
