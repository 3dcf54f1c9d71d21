"""ia_ln_fwd_rows: the LayerNorm tail z = residual + dropout(x + bias), y = LN(z) with a row filter, against ia_ln_fwd on the same
inputs.  M = 1030 rows (no multiple of the 4 rows of a workgroup or of 64), H = 768 (one and a half 512-column slabs) and 1024; dropout
0 and 0.1; with z_out, without it and with z_out written over x; a ragged mask, every row live and every row dead.

Live rows of y, z, mean and rstd must be torch.equal to the unfiltered call's (the dropout stream is indexed by position, so a live row
draws what it draws there); dead rows must be zeros everywhere; and the inputs of the dead rows are NaN, so a kernel that read one of
them into any output would show."""
import pytest
import torch

pytestmark = pytest.mark.gpu

M = 1030


def row_masks():
    g = torch.Generator().manual_seed(3)
    ragged = torch.zeros(M, dtype=torch.uint8)
    for b in range(0, M, 103):                          # right-padded sequences of 103 positions, ragged lengths
        ragged[b: b + int(torch.randint(1, 104, (1,), generator=g))] = 1
    ragged[M - 1] = 1; ragged[M - 2] = 0
    return {"ragged": ragged, "all_live": torch.ones(M, dtype=torch.uint8), "all_dead": torch.zeros(M, dtype=torch.uint8)}


@pytest.mark.parametrize("z_mode", ["z_out", "no_z", "in_place"])
@pytest.mark.parametrize("drop_p", [0.0, 0.1])
@pytest.mark.parametrize("H", [768, 1024])
def test_ln_fwd_rows(gpu, H, drop_p, z_mode):
    from item_alignment_amd import ops
    g = torch.Generator().manual_seed(17 + H)
    x = torch.randn(M, H, generator=g).to(gpu).to(torch.bfloat16)
    res = torch.randn(M, H, generator=g).to(gpu).to(torch.bfloat16)
    bias = (torch.randn(H, generator=g) * 0.1).to(gpu)
    gamma = (1 + 0.1 * torch.randn(H, generator=g)).to(gpu)
    beta = (0.1 * torch.randn(H, generator=g)).to(gpu)
    kw = dict(bias=bias, drop_p=drop_p, seed=123, stream_id=7)
    y0, z0, mean0, rstd0 = ops.ln_fwd(x, gamma, beta, 1e-12, residual=res, write_z=True, **kw)
    for name, live_cpu in row_masks().items():
        live = live_cpu.to(gpu)
        lv = live.bool()
        nan = torch.tensor(float("nan"), device=gpu, dtype=torch.bfloat16)
        xin = torch.where(lv[:, None], x, nan).contiguous()             # dead rows: NaN in both input streams
        rin = torch.where(lv[:, None], res, nan).contiguous()
        y, z, mean, rstd = ops.ln_fwd_rows(xin, gamma, beta, 1e-12, live, residual=rin, write_z=z_mode != "no_z", in_place=z_mode == "in_place", **kw)
        assert torch.equal(y[lv], y0[lv]), name
        assert torch.equal(mean[lv], mean0[lv]) and torch.equal(rstd[lv], rstd0[lv]), name
        outs = [y, mean, rstd]
        if z is not None:
            assert torch.equal(z[lv], z0[lv]), name
            outs.append(z)
        for t in outs:
            assert torch.isfinite(t.float()).all(), name
            if (~lv).any():
                assert t[~lv].float().abs().max().item() == 0.0, name
    # NULL = ia_ln_fwd
    y, z, mean, rstd = ops.ln_fwd_rows(x, gamma, beta, 1e-12, None, residual=res, **kw)
    assert torch.equal(y, y0) and torch.equal(z, z0) and torch.equal(mean, mean0) and torch.equal(rstd, rstd0)
