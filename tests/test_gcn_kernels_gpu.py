"""The graph-encoder kernels (csrc/gcn.hip) per element against the fp64 restatement of tests/gcn_reference.py:
|got - ref| <= tau * S, S = the same expression on absolute values, tau = (n + 4) * 2^-24 with n the longest fp32 sum feeding the
element (derived, not measured): the row degree for the propagate kernels, C for h @ W, F for the input layer, the slab length
IA_GCN_SLAB_ROWS for the weight gradients (their slabs are joined in fp64 and rounded once).  The +4 covers the roundings outside the
sum: the constants (1 - alpha) / keep, alpha, beta as floats, the final blend.  GCN-BOUND lines (run with -s) print the observed
max |err| / S in units of 2^-24 next to n + 4.

tau also has to lie below the dropped-contribution level -- the relative change of an element if one neighbour (one term of its
sum) were lost, 1 / n for terms of equal size -- or the bound could not see a missing edge.  That holds for every case except the
row of degree >= 20000 of the split-row cases ('hub': a hub row of A for the forward; 'hubT': the same graph transposed, a hub row of
A^T for the backward), where (n + 4) * 2^-24 ~ 1.2e-3 > 1 / n = 5e-5 cannot be avoided by construction; the checks that sum over
that row are named in LOSSY_BY_CONSTRUCTION, (case, check) by (case, check), and are the only exception.

Every 'mixed' case carries rows of A AND of A^T beyond IA_GCN_LONG_ROW (512) neighbours ('hub' only of A, 'hubT' only of A^T), so the
workgroup-per-row path (16 chunks, LDS join, the finish with the output-row mask, the dx0 accumulate flag and the dx = NULL form) runs
in both directions at every width and index type; the test asserts that the long-row lists it relies on are non-empty.
"""
import numpy as np
import pytest
import torch

import gcn_reference as R

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
SLAB = 1024
LOSSY_BY_CONSTRUCTION = (("hub", "propagate_fwd"), ("hub", "fwd_no_list"), ("hubT", "propagate_bwd"), ("hubT", "bwd_no_list"),
                         ("hubT", "bwd_joined"))


def lib_():
    from item_alignment_amd import _lib
    return _lib.load()


def st():
    from item_alignment_amd._lib import stream_ptr
    return stream_ptr()


def P(t):
    return None if t is None else t.data_ptr()


def make_graph(kind, N, rs, signed_vals):
    """(row, col, val-or-None) COO lists, unsymmetric.  Row 0 has degree 0, row 1 degree 1.  'mixed': every 50th row has 600
    neighbours and every second row points at node 7, so column 7 (a row of A^T) has more than 512 entries too.  'hub': row 2 has
    >= 20000 neighbours beside rows of degree 5; 'hubT' is that graph transposed (a hub column: the long row is in A^T)."""
    rows, cols = [1], [int(rs.randint(N))]
    for i in range(2, N):
        if kind in ("hub", "hubT"):
            deg = 20000 + 37 if i == 2 else 5
        else:
            deg = int(rs.randint(2, 30)) if i % 50 else 600     # some rows beyond IA_GCN_LONG_ROW (512) in every case
        deg = min(deg, N)
        c = rs.choice(N, size=deg, replace=False)
        if kind == "mixed" and i % 2 == 0 and 7 not in c:
            c[0] = 7
        rows += [i] * deg
        cols += c.tolist()
    row, col = np.asarray(rows), np.asarray(cols)
    if kind == "hubT":
        row, col = col, row
    val = rs.uniform(-1, 1, size=len(row)).astype(np.float32) if signed_vals else None
    return row, col, val


def build(kind, N, rs, signed_vals, col64):
    from item_alignment_amd.models.graph import load_adjacency
    row, col, val = make_graph(kind, N, rs, signed_vals)
    ei = torch.from_numpy(np.stack([col, row]))                      # PyG order: edge_index[0] = source j, [1] = target i
    adj = load_adjacency((ei, None if val is None else torch.from_numpy(val)), num_nodes=N, device="cuda")
    if col64:
        adj.col, adj.col_t = adj.col.long(), adj.col_t.long()
    A = torch.sparse_coo_tensor(torch.from_numpy(np.stack([row, col])), torch.ones(len(row), dtype=R.F64) if val is None
                                else torch.from_numpy(val).double(), (N, N)).coalesce()
    deg = torch.from_numpy(np.bincount(row, minlength=N)).double()
    deg_t = torch.from_numpy(np.bincount(col, minlength=N)).double()
    return adj, A, deg, deg_t


def check(name, got, ref, S, n, case):
    """n: longest sum per element (a number, or a tensor broadcastable against the rows)."""
    got = got.double().cpu()
    n_t = n if torch.is_tensor(n) else torch.tensor(float(n), dtype=R.F64)
    tau = (n_t + 4) * U
    n_max = float(n_t.max())
    if (case, name) not in LOSSY_BY_CONSTRUCTION:
        assert (n_max + 4) * U < 1.0 / max(n_max, 1.0), (name, case, "tau above the dropped-contribution level")
    err = (got - ref).abs()
    ratio = float((err / S.clamp_min(1e-300)).max() / U) if S.numel() else 0.0
    print(f"GCN-BOUND {case:8s} {name:14s} max|err|/S = {ratio:8.2f} * 2^-24   (n + 4 = {n_max + 4:.0f})")
    bad = err > tau * S + 1e-300
    assert not bool(bad.any()), (name, case, ratio, n_max + 4)


CASES = [
    # case, kind, N, C, signed values, int64 col, p
    ("c32", "mixed", 1037, 32, False, False, 0.0),
    ("c128", "mixed", 2051, 128, True, False, 0.1),
    ("c128i64", "mixed", 1037, 128, False, True, 0.1),
    ("c160", "mixed", 1037, 160, True, True, 0.0),
    ("c512", "mixed", 1037, 512, True, False, 0.1),
    ("hub", "hub", 21013, 128, True, False, 0.1),
    ("hubT", "hubT", 21013, 128, True, False, 0.1),
]


@pytest.mark.parametrize("case,kind,N,C,signed,col64,p", CASES)
def test_propagate(case, kind, N, C, signed, col64, p):
    lib = lib_()
    rs = np.random.RandomState(len(case) * 1000 + N + C)
    adj, A, deg, deg_t = build(kind, N, rs, signed, col64)
    assert N % 16
    if kind == "hubT":
        assert int(deg_t[2]) >= 20000 and int(deg_t[3]) == 5 and int(deg_t[0]) == 0 and int(deg_t[1]) == 1
        assert adj.long_rows_t.tolist() == [2]
    else:
        assert int(deg[0]) == 0 and int(deg[1]) == 1
        assert adj.long_rows.numel() > 0
    if kind == "hub":
        assert int(deg[2]) >= 20000 and int(deg[3]) == 5 and adj.long_rows.tolist() == [2]
    if kind == "mixed":
        assert adj.long_rows_t.numel() > 0 and int(deg_t.max()) > 512       # the split-row path of the backward runs
    x = torch.from_numpy(rs.standard_normal((N, C)).astype(np.float32)).cuda()
    x0 = torch.from_numpy(rs.standard_normal((N, C)).astype(np.float32)).cuda()
    alpha, seed, sid = 0.1, 777 + N, 3001
    keep, scale = R.keep_mask(seed, sid, N * C, p)
    keep = keep.view(N, C)
    lr = adj.long_rows
    outs = []
    for _ in range(2):
        h = torch.full((N, C), 7.0, device="cuda")
        rc = lib.ia_gcn_propagate_fwd(P(adj.rowptr), P(adj.col), int(col64), P(adj.val), P(x), P(x0), P(h), N, C, alpha, p, seed, sid,
                                      P(lr) if lr.numel() else None, lr.numel(), st())
        assert rc == 0
        outs.append(h)
    torch.cuda.synchronize()
    assert torch.equal(outs[0], outs[1])
    ref, S = R.propagate_fwd(A, x.double().cpu(), x0.double().cpu(), float(np.float32(alpha)), keep, scale)
    check("propagate_fwd", outs[0], ref, S, deg.view(N, 1), case)
    # without the long-row list every row is summed by one wave: same bound, same values up to it
    h1 = torch.empty((N, C), device="cuda")
    assert lib.ia_gcn_propagate_fwd(P(adj.rowptr), P(adj.col), int(col64), P(adj.val), P(x), P(x0), P(h1), N, C, alpha, p, seed, sid, None, 0, st()) == 0
    check("fwd_no_list", h1, ref, S, deg.view(N, 1), case)

    # backward on the transposed structure (A is unsymmetric); dx0 with prior contents, and the dx-joins-dx0 form.  Except in 'hub'
    # (in-degrees ~ 6) the list of long rows of A^T is not empty: those rows take the workgroup-per-row path
    assert kind == "hub" or adj.long_rows_t.numel() > 0
    dh = torch.from_numpy(rs.standard_normal((N, C)).astype(np.float32)).cuda()
    prior = torch.from_numpy(rs.standard_normal((N, C)).astype(np.float32)).cuda()
    lrt = adj.long_rows_t
    res = []
    for _ in range(2):
        dx = torch.full((N, C), 7.0, device="cuda")
        dx0 = prior.clone()
        rc = lib.ia_gcn_propagate_bwd(P(adj.rowptr_t), P(adj.col_t), int(col64), P(adj.val_t), P(dh), P(dx), P(dx0), 1, N, C, alpha, p, seed, sid,
                                      P(lrt) if lrt.numel() else None, lrt.numel(), st())
        assert rc == 0
        res.append((dx, dx0))
    dx0_only = torch.full((N, C), 7.0, device="cuda")
    assert lib.ia_gcn_propagate_bwd(P(adj.rowptr_t), P(adj.col_t), int(col64), P(adj.val_t), P(dh), None, P(dx0_only), 0, N, C, alpha, p, seed, sid,
                                    P(lrt) if lrt.numel() else None, lrt.numel(), st()) == 0
    torch.cuda.synchronize()
    assert torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][1], res[1][1])
    rdx, Sx, rdx0, S0 = R.propagate_bwd(A, dh.double().cpu(), float(np.float32(alpha)), keep, scale, prior.double().cpu())
    check("propagate_bwd", res[0][0], rdx, Sx, deg_t.view(N, 1), case)
    check("bwd_dx0", res[0][1], rdx0, S0, 1, case)
    dx1, dx01 = torch.empty((N, C), device="cuda"), prior.clone()
    assert lib.ia_gcn_propagate_bwd(P(adj.rowptr_t), P(adj.col_t), int(col64), P(adj.val_t), P(dh), P(dx1), P(dx01), 1, N, C, alpha, p, seed, sid,
                                    None, 0, st()) == 0
    check("bwd_no_list", dx1, rdx, Sx, deg_t.view(N, 1), case)
    assert torch.equal(dx01, res[0][1])
    _, _, r0, s0 = R.propagate_bwd(A, dh.double().cpu(), float(np.float32(alpha)), keep, scale, None)
    check("bwd_joined", dx0_only, rdx + r0, Sx + s0, deg_t.view(N, 1) + 1, case)


@pytest.mark.parametrize("case,N,C,p", [("c32", 1037, 32, 0.0), ("c128", 2051, 128, 0.1), ("c160", 1037, 160, 0.1), ("c512", 1037, 512, 0.0)])
def test_mix(case, N, C, p):
    lib = lib_()
    rs = np.random.RandomState(N + C)
    h = torch.from_numpy(rs.standard_normal((N, C)).astype(np.float32)).cuda()
    W = torch.from_numpy((rs.standard_normal((C, C)) / np.sqrt(C)).astype(np.float32)).cuda()
    beta, seed, sid = float(np.float32(np.log(0.5 / 2 + 1))), 991, 3005
    keep, scale = R.keep_mask(seed, sid, N * C, p)
    outs = []
    for _ in range(2):
        out = torch.full((N, C), 7.0, device="cuda")
        assert lib.ia_gcn_mix_fwd(P(h), P(W), P(out), N, C, beta, p, seed, sid, st()) == 0
        outs.append(out)
    torch.cuda.synchronize()
    assert torch.equal(outs[0], outs[1])
    ref, S, pre = R.mix_fwd(h.double().cpu(), W.double().cpu(), beta, keep.view(N, C), scale)
    # an element whose pre-activation is within the bound of zero may land on either side of the relu: |got - ref| <= tau S still holds
    check("mix_fwd", outs[0], ref, S, C, case)

    out = outs[0]
    dout = torch.from_numpy(rs.standard_normal((N, C)).astype(np.float32)).cuda()
    ws_bytes = int(lib.ia_gcn_workspace_bytes(N, C, 0))
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device="cuda")
    prior = torch.from_numpy(rs.standard_normal((C, C)).astype(np.float32)).cuda()
    res = []
    for _ in range(2):
        dh = torch.full((N, C), 7.0, device="cuda")
        dW = prior.clone()
        assert lib.ia_gcn_mix_bwd(P(dout), P(out), P(h), P(W), P(dh), P(dW), N, C, beta, p, P(ws), ws_bytes, st()) == 0
        res.append((dh, dW))
    torch.cuda.synchronize()
    assert torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][1], res[1][1])
    rdh, Sh, rdW, SW = R.mix_bwd(dout.double().cpu(), out.double().cpu(), h.double().cpu(), W.double().cpu(), beta, scale)
    check("mix_bwd_dh", res[0][0], rdh, Sh, C, case)
    check("mix_bwd_dW", res[0][1], rdW + prior.double().cpu(), SW + prior.double().cpu().abs(), min(SLAB, N), case)


@pytest.mark.parametrize("case,N,F,C,p", [("f64", 1037, 64, 32, 0.0), ("f1024", 2051, 1024, 128, 0.1), ("f100", 1037, 100, 160, 0.1)])
def test_input_layer(case, N, F, C, p):
    lib = lib_()
    rs = np.random.RandomState(N + F)
    X = torch.from_numpy(rs.standard_normal((N, F)).astype(np.float32)).cuda()
    W = torch.from_numpy((rs.standard_normal((C, F)) / np.sqrt(F)).astype(np.float32)).cuda()
    b = torch.from_numpy(rs.standard_normal(C).astype(np.float32)).cuda()
    seed, sid = 4242, 3000
    keep, scale = R.keep_mask(seed, sid, N * F, p)
    keep = keep.view(N, F)
    outs = []
    for _ in range(2):
        x0 = torch.full((N, C), 7.0, device="cuda")
        assert lib.ia_gcn_input_fwd(P(X), P(W), P(b), P(x0), N, F, C, p, seed, sid, st()) == 0
        outs.append(x0)
    torch.cuda.synchronize()
    assert torch.equal(outs[0], outs[1])
    ref, S = R.input_fwd(X.double().cpu(), W.double().cpu(), b.double().cpu(), keep, scale)
    check("input_fwd", outs[0], ref, S, F + 1, case)

    x0 = outs[0]
    dx0 = torch.from_numpy(rs.standard_normal((N, C)).astype(np.float32)).cuda()
    ws_bytes = int(lib.ia_gcn_workspace_bytes(N, C, F))
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device="cuda")
    pW = torch.from_numpy(rs.standard_normal((C, F)).astype(np.float32)).cuda()
    pb = torch.from_numpy(rs.standard_normal(C).astype(np.float32)).cuda()
    res = []
    for _ in range(2):
        dW, db = pW.clone(), pb.clone()
        assert lib.ia_gcn_input_bwd(P(dx0), P(x0), P(X), P(dW), P(db), N, F, C, p, seed, sid, P(ws), ws_bytes, st()) == 0
        res.append((dW, db))
    torch.cuda.synchronize()
    assert torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][1], res[1][1])
    rW, SW, rb, Sb = R.input_bwd(dx0.double().cpu(), x0.double().cpu(), X.double().cpu(), keep, scale)
    check("input_bwd_dW", res[0][0], rW + pW.double().cpu(), SW + pW.double().cpu().abs(), min(SLAB, N), case)
    check("input_bwd_db", res[0][1], rb + pb.double().cpu(), Sb + pb.double().cpu().abs(), min(SLAB, N), case)


@pytest.mark.parametrize("p", [0.0, 0.1])
def test_pair_gather_and_scatter_with_repeated_nodes(p):
    lib = lib_()
    rs = np.random.RandomState(5)
    N, C, Rr = 300, 128, 16
    x = torch.from_numpy(rs.standard_normal((N, C)).astype(np.float32)).cuda()
    idx_h = np.asarray([5, 9, 5, 200, 9, 5, 0, 299, 17, 17, 3, 4, 5, 6, 7, 8], dtype=np.int32)
    idx = torch.from_numpy(idx_h).cuda()
    seed, sid = 31337, 3100
    keep, scale = R.keep_mask(seed, sid, Rr * C, p)
    k = keep.view(Rr, C) * scale
    out = torch.empty((Rr, C), device="cuda")
    assert lib.ia_gcn_pair_gather_fwd(P(x), P(idx), P(out), Rr, C, N, p, seed, sid, st()) == 0
    ref = x.double().cpu()[torch.from_numpy(idx_h).long()] * k
    check("pair_gather", out, ref, ref.abs(), 0, "pairs")
    dout = torch.from_numpy(rs.standard_normal((Rr, C)).astype(np.float32)).cuda()
    order = torch.argsort(idx, stable=True).to(torch.int32)
    prior = torch.from_numpy(rs.standard_normal((N, C)).astype(np.float32)).cuda()
    res = []
    for _ in range(2):
        dnode = prior.clone()
        assert lib.ia_gcn_pair_scatter_bwd(P(dout), P(idx), P(order), P(dnode), Rr, C, N, p, seed, sid, st()) == 0
        res.append(dnode)
    torch.cuda.synchronize()
    assert torch.equal(res[0], res[1])
    g = dout.double().cpu() * k
    rd = prior.double().cpu().clone()
    rd.index_add_(0, torch.from_numpy(idx_h).long(), g)
    Sd = prior.double().cpu().abs()
    Sd.index_add_(0, torch.from_numpy(idx_h).long(), g.abs())
    check("pair_scatter", res[0], rd, Sd, 4 + 1, "pairs")           # node 5 occurs four times, plus the prior contents
