"""ia_vocab_ce_fwd / ia_vocab_ce_bwd through the C ABI against the fp64 reference of tests/vocab_ce_reference.py computed from the same
fp32 logits, element by element.  The bars are derived there, not measured:

  * lse, loss_row and the mean are fp32 sums: |got - want| <= the reference's bound, built from the chain length c of the kernel's
    summation (vocab_ce_reference.row_chain / mean_chain, read off csrc/vocab_ce.hip: c = ceil(V / 1024) + 12 per row) and the 1 ulp of
    expf / logf;
  * dlogits is a bf16 output of fp32 arithmetic: |got - want| <= 2^-8 |want| + the fp32 bound;
  * wherever the bound is zero -- ignored rows, rows whose label is outside the vocabulary, the columns V .. ldg-1 -- the output is
    exactly zero.
Every helper prints the largest error it saw as a fraction of its bound (`-s` shows them); that figure is recorded, never used to set
a bound.
"""
import math

import pytest
import torch

import vocab_ce_reference as R

pytestmark = pytest.mark.gpu

F64, F32, BF16 = torch.float64, torch.float32, torch.bfloat16
ERR_ARG, ERR_WS = -1, -3
DLOSS = 0.75

#         M,   V,     ld,    ldg
SHAPES = [(3, 21128, 21128, 21128),      # the real width
          (1, 8, 8, 8),                  # narrower than one wave's vector
          (5, 1003, 1004, 1008),         # odd V: the pad columns of logits hold NaN, those of dlogits garbage
          (257, 1000, 1000, 1000),       # row-grid edge
          (4, 4100, 4100, 4104),         # mid-size tail
          (8, 21128, 21128, 21128)]      # every kind of row below at the real width


def build(M, V, ld, ldg, seed):
    """Row r is of kind r % 8: 0 random; 1 all-equal; 2 one logit 80 above the rest, labelled; 3 magnitudes 1e4 and -1e4; 4 label at
    column 0; 5 label at V - 1; 6 ignored; 7 one logit 80 above the rest, another column labelled."""
    g = torch.Generator().manual_seed(seed)
    x = torch.full((M, ld), float("nan"), dtype=F32)
    y = torch.randint(0, V, (M,), generator=g)
    for r in range(M):
        k = r % 8
        row = torch.randn(V, generator=g) * 3.0
        if k == 1:
            row = torch.full((V,), 2.5)
        elif k in (2, 7):
            row = torch.randn(V, generator=g)
            c = int(torch.randint(0, V, (1,), generator=g))
            row[c] = row.max() + 80.0
            y[r] = c if k == 2 else (c + 1) % V
        elif k == 3:
            row = torch.where(torch.rand(V, generator=g) < 0.5, torch.tensor(1e4), torch.tensor(-1e4)) + torch.randn(V, generator=g)
        elif k == 4:
            y[r] = 0
        elif k == 5:
            y[r] = V - 1
        elif k == 6:
            y[r] = -1
        x[r, :V] = row
    return x, y


@pytest.fixture(scope="module")
def lib(gpu):
    from item_alignment_amd import _lib
    return _lib.load()


def st():
    from item_alignment_amd import _lib
    return _lib.stream_ptr()


def run(lib, x, y, V, ldg, dloss=DLOSS):
    """-> lse, loss_row, loss [2], dlogits (device tensors) of one forward + backward; dlogits starts as garbage"""
    from item_alignment_amd import _lib
    M, ld = x.shape
    xd, yd = x.cuda(), y.cuda()
    lse = torch.full((M,), 7.0, device="cuda")
    loss_row = torch.full((M,), 7.0, device="cuda")
    loss = torch.full((2,), 7.0, device="cuda")
    ws_bytes = lib.ia_vocab_ce_workspace_bytes(M)
    ws = torch.empty(ws_bytes, device="cuda", dtype=torch.uint8)
    _lib.check(lib.ia_vocab_ce_fwd(xd.data_ptr(), ld, yd.data_ptr(), lse.data_ptr(), loss_row.data_ptr(), loss.data_ptr(), M, V,
                                   ws.data_ptr(), ws_bytes, st()), "ia_vocab_ce_fwd")
    dl = torch.tensor([dloss], device="cuda", dtype=F32)
    g = torch.full((M, ldg), 123.0, device="cuda", dtype=BF16)
    _lib.check(lib.ia_vocab_ce_bwd(xd.data_ptr(), ld, yd.data_ptr(), lse.data_ptr(), loss.data_ptr(), dl.data_ptr(), g.data_ptr(), ldg, M, V,
                                   st()), "ia_vocab_ce_bwd")
    torch.cuda.synchronize()
    return lse, loss_row, loss, g


def close(name, got, want, bound):
    """|got - want| <= bound element by element, exact where the bound is zero, NaN exactly where the reference has NaN"""
    got, want, bound = got.detach().cpu().to(F64).reshape(-1), want.to(F64).reshape(-1), bound.to(F64).reshape(-1)
    nan = torch.isnan(want)
    assert torch.equal(torch.isnan(got), nan), (name, "NaN in other places than the reference")
    err = (got - want).abs()[~nan]
    bound = bound[~nan]
    assert torch.isfinite(err).all(), (name, "non-finite output")
    exact = bound == 0
    assert (err[exact] == 0).all(), (name, "an element whose bound is zero is not exact", float(err[exact].max()))
    r = float((err[~exact] / bound[~exact]).max()) if (~exact).any() else 0.0
    print(f"[vocab_ce] {name}: max error / bound = {r:.3f}")
    assert r <= 1.0, (name, r)


def check_case(lib, x, y, V, ldg, tag):
    lse, loss_row, loss, g = run(lib, x, y, V, ldg)
    f = R.forward(x, y, V)
    close(f"{tag} lse (c = {R.row_chain(V)})", lse, f["lse"], f["lse_bound"])
    close(f"{tag} loss_row", loss_row, f["loss_row"], f["loss_row_bound"])
    close(f"{tag} mean (c = {R.mean_chain(x.shape[0])})", loss[0], f["mean"], f["mean_bound"])
    assert float(loss[1]) == f["n_live"]
    want, fp32_bound = R.backward(x, y, V, ldg, dloss=DLOSS, fwd=f)
    close(f"{tag} dlogits", g, want, R.BF16_ULP * want.abs() + fp32_bound)
    assert (g[:, V:] == 0).all()
    return lse, loss_row, loss, g


@pytest.mark.parametrize("M,V,ld,ldg", SHAPES)
def test_forward_and_backward_against_fp64(lib, M, V, ld, ldg):
    x, y = build(M, V, ld, ldg, seed=100 + M + V)
    lse, loss_row, _, g = check_case(lib, x, y, V, ldg, f"{M}x{V}")
    for r in range(M):
        if r % 8 == 1:          # all-equal logits: lse = x + ln V
            assert abs(float(lse[r]) - (2.5 + math.log(V))) <= float(R.forward(x[r:r + 1], y[r:r + 1], V)["lse_bound"][0])
        if r % 8 == 6:          # ignored rows
            assert float(loss_row[r]) == 0.0 and (g[r] == 0).all()


def test_all_rows_ignored(lib):
    x, _ = build(5, 1003, 1004, 1008, seed=5)
    y = torch.full((5,), -1)
    _, loss_row, loss, g = check_case(lib, x, y, 1003, 1008, "all ignored")
    assert math.isnan(float(loss[0])) and float(loss[1]) == 0.0
    assert (loss_row == 0).all() and (g == 0).all()


@pytest.mark.parametrize("M,V,ld,ldg", [(5, 1003, 1004, 1008), (3, 21128, 21128, 21128)])
def test_label_outside_the_vocabulary(lib, M, V, ld, ldg):
    """NaN loss, nothing out of bounds (a label far outside: an unchecked read would land in another allocation or fault), zero
    gradient row; the other rows keep their gradients"""
    x, y = build(M, V, ld, ldg, seed=9)
    y[0], y[2] = V, 2 ** 40
    _, loss_row, loss, g = check_case(lib, x, y, V, ldg, "label >= V")
    assert math.isnan(float(loss_row[0])) and math.isnan(float(loss_row[2])) and math.isnan(float(loss[0]))
    assert (g[0] == 0).all() and (g[2] == 0).all() and (g[1] != 0).any()


@pytest.mark.parametrize("M,V,ld,ldg", [(257, 1000, 1000, 1000), (3, 21128, 21128, 21128)])
def test_two_runs_are_bit_identical(lib, M, V, ld, ldg):
    x, y = build(M, V, ld, ldg, seed=21)
    a, b = run(lib, x, y, V, ldg), run(lib, x, y, V, ldg)
    for name, u, v in zip(("lse", "loss_row", "loss", "dlogits"), a, b):
        iv = torch.int16 if u.dtype == BF16 else torch.int32
        assert torch.equal(u.view(iv), v.view(iv)), name


def test_argument_checks_return_their_codes(lib):
    """every refusal comes before a launch: the outputs keep what they held"""
    M, V = 4, 16
    x = torch.zeros((M, V), device="cuda")
    y = torch.zeros(M, device="cuda", dtype=torch.int64)
    out = torch.full((2 * M + 2,), 7.0, device="cuda")
    lse, row, loss = out[:M], out[M:2 * M], out[2 * M:]
    ws_bytes = lib.ia_vocab_ce_workspace_bytes(M)
    assert ws_bytes >= 8 and lib.ia_vocab_ce_workspace_bytes(0) == 0 and lib.ia_vocab_ce_workspace_bytes(1025) >= 16
    ws = torch.empty(ws_bytes, device="cuda", dtype=torch.uint8)
    g = torch.full((M, V), 7.0, device="cuda", dtype=BF16)
    dl = torch.ones(1, device="cuda")
    X, Y, L, Rw, Lo, W, G, D = (t.data_ptr() for t in (x, y, lse, row, loss, ws, g, dl))

    def fwd(x=X, ld=V, y=Y, l=L, r=Rw, lo=Lo, m=M, v=V, w=W, wb=ws_bytes):
        return lib.ia_vocab_ce_fwd(x, ld, y, l, r, lo, m, v, w, wb, st())

    def bwd(x=X, ld=V, y=Y, l=L, lo=Lo, d=D, g=G, ldg=V, m=M, v=V):
        return lib.ia_vocab_ce_bwd(x, ld, y, l, lo, d, g, ldg, m, v, st())

    for kw in (dict(x=None), dict(y=None), dict(l=None), dict(r=None), dict(lo=None), dict(m=0), dict(v=0), dict(m=-1), dict(v=-3),
               dict(ld=V - 4), dict(ld=V + 2), dict(ld=V + 1)):
        assert fwd(**kw) == ERR_ARG, kw
    assert fwd(w=None) == ERR_WS and fwd(wb=ws_bytes - 1) == ERR_WS and fwd(wb=0) == ERR_WS
    for kw in (dict(x=None), dict(y=None), dict(l=None), dict(lo=None), dict(d=None), dict(g=None), dict(m=0), dict(v=0), dict(ld=V - 4),
               dict(ld=V + 2), dict(ldg=V - 8), dict(ldg=V + 4), dict(ldg=V + 1)):
        assert bwd(**kw) == ERR_ARG, kw
    torch.cuda.synchronize()
    assert (out == 7.0).all() and (g == 7.0).all()
    assert fwd() == 0 and bwd() == 0
    torch.cuda.synchronize()
    assert abs(float(loss[0]) - math.log(V)) < 1e-5 and float(loss[1]) == M
