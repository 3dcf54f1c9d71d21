"""The knowledge-graph pretraining kernels (csrc/kgpretrain.hip) against the fp64 reference of tests/kgpt_reference.py, per element,
at the production widths and at the edges of the GEMM tiles, the lane loops and the segment-sum pieces: ia_kgpt_score in all its
(model, norm, mode) forms, ia_kgpt_adam_l2 and ia_kgpt_row_normalize.

Every score case starts from non-zero gradients (the kernels accumulate) and checks |got - before - ref| <= tau * S + U per element
(S, U from the reference; plus one fp32 rounding of the final add), that table rows without a contribution are bit-identical to
before, and that a second identical call repeats the first bit for bit.  The observed max |got - ref| / S of every check is printed
as a `KGPT-BOUND` line (run with -s to see them)."""
import math
import os
import re

import numpy as np
import pytest
import torch

import kgpt_reference as R
from item_alignment_amd import _lib
from item_alignment_amd._lib import stream_ptr
from item_alignment_amd.models import kg_pretrain as K

pytestmark = pytest.mark.gpu
TAU = 1e-5                 # scores and row gradients
TAU_DP_LONG = 1e-4         # dP once 2B >= 8192 (each split-K partial sums 2B / 16 terms in sequence)
EPS32 = R.EPS32


def report(case, what, q, tau, drop=None):
    extra = "" if drop is None else f" drop={drop:.2e}"
    print(f"KGPT-BOUND {case} {what} max|err|/S={q:.3e} tau={tau:.0e}{extra}")


def drop_level(ref, table):
    """The dropped-contribution level of a table gradient: the 1st percentile, over the occurrences with a non-zero gradient, of the
    relative error that losing that one occurrence would leave (max over its row of |contribution| / S)."""
    return torch.quantile(ref["drop_" + table].float().cpu(), 0.01).item()


def check(case, what, got, before, ref, S, tau, U=None, drop=None):
    """|got - before - ref| <= tau * S + U + 1 ulp-ish of the final add, per element; S == 0 -> got is before, bit for bit.  With a
    dropped-contribution level, tau must lie below it (else losing a contribution could pass)."""
    got64, b64 = got.double(), before.double()
    err = (got64 - b64 - ref).abs() - (0 if U is None else U) - EPS32 * got64.abs()
    untouched = S == 0
    if U is not None:
        untouched &= U == 0
    assert torch.equal(got[untouched], before[untouched]), f"{case} {what}: an element without contribution changed"
    q = (err.clamp_min(0) / torch.where(S > 0, S, torch.ones_like(S))).max().item()
    report(case, what, q, tau, drop)
    assert drop is None or tau < drop, f"{case} {what}: tau {tau:.0e} is not below the dropped-contribution level {drop:.2e}"
    assert q <= tau, f"{case} {what}: max |got - ref| / S = {q:.3e} > tau {tau:.0e}"
    return q


def rand_tables(n_ent, n_rel, D, proj, dev, seed):
    g = torch.Generator(device="cpu").manual_seed(seed)
    scale = torch.exp(torch.randn(n_ent, 1, generator=g) * 1.5)          # row norms over ~ e^+-4: the normaliser matters
    ent = (torch.randn(n_ent, D, generator=g) * scale).to(dev)
    rel = (torch.randn(n_rel, D, generator=g) / math.sqrt(D)).to(dev)
    P = (torch.randn(D, D, generator=g) / math.sqrt(D)).to(dev) if proj else None
    return ent, rel, P


def make_model(kind, norm, ent, rel, P):
    cls = K.PKGMPretrainModel if kind == "pkgm" else K.TransEPretrainModel
    n_ent, D = ent.shape
    m = cls(4, 1, 1, dissimilarity_type=norm)                            # tiny host init, then the test's tables
    m.emb_dim, m.n_ent, m.n_rel = D, n_ent, rel.shape[0]
    m.ent_emb = torch.nn.Embedding.from_pretrained(ent.clone(), freeze=False)
    m.rel_emb = torch.nn.Embedding.from_pretrained(rel.clone(), freeze=False)
    if P is not None:
        m.proj_mat = torch.nn.Linear(1, 1, bias=False)
        m.proj_mat.weight = torch.nn.Parameter(P.clone())
    return m


def sentinel_grads(m, seed):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return [(torch.randn(p.shape, generator=g) * 1e-2).to(p.device) for p in m.tables()]


def set_grads(m, before):
    for p, b in zip(m.tables(), before):
        p.grad = b.clone()


def rand_ids(B, n_ent, n_rel, dev, seed):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return [torch.randint(0, n, (B,), generator=g).to(dev) for n in (n_ent, n_ent, n_rel, n_ent, n_ent)]


def pick_margin(ent, rel, P, ids, norm):
    """A margin (fp32) whose hinge decisions are all >= 1e-4 away from a tie in fp64, about half of the pairs active."""
    pos, neg = R.scores(ent, rel, P, *ids, 2 if norm == "L2" else 1)
    d = (pos - neg).sort().values.cpu()
    if d.numel() == 1:
        return R.f32(d[0].item() + 0.5)
    lo, hi = d.numel() // 4, max(d.numel() * 3 // 4, d.numel() // 4 + 1)
    gaps = d[lo + 1:hi + 1] - d[lo:hi]
    i = lo + int(gaps.argmax())
    return R.f32((d[i].item() + d[i + 1].item()) / 2)


def margin_case(case, kind, norm, D, B, n_ent, n_rel, dev, seed, ids=None, m=None, tabs=None):
    """MARGIN-mode step against fp64, from sentinel gradients, run twice: returns the model (its _ws reused by the caller)."""
    nrm = 2 if norm == "L2" else 1
    ent, rel, P = tabs if tabs is not None else rand_tables(n_ent, n_rel, D, kind == "pkgm", dev, seed)
    if m is None:
        m = make_model(kind, norm, ent, rel, P)
    ids = ids if ids is not None else rand_ids(B, n_ent, n_rel, dev, seed + 1)
    margin = pick_margin(ent, rel, P, ids, norm)
    ref = R.score_step(ent, rel, P, *ids, nrm, margin=margin, sign_tol=nrm == 1)
    assert (margin - ref["pos"] + ref["neg"]).abs().min().item() >= 1e-4, "a hinge decision lies within 1e-4 of a tie"
    before = sentinel_grads(m, seed + 2)
    runs = []
    for _ in range(2):
        set_grads(m, before)
        loss, pos, neg = m.margin_step(*ids, margin=margin)
        torch.cuda.synchronize()
        runs.append([pos.clone(), neg.clone(), loss.clone()] + [p.grad.clone() for p in m.tables()])
    for a, b in zip(*runs):
        assert torch.equal(a, b), f"{case}: a second identical call differs"
    pos, neg, loss, *grads = runs[0]
    zero = torch.zeros_like(pos)
    check(case, "pos", pos, zero, ref["pos"], ref["S_pos"], TAU)
    check(case, "neg", neg, zero, ref["neg"], ref["S_neg"], TAU)
    check(case, "loss", loss, torch.zeros_like(loss), ref["loss"].reshape(1), (ref["S_pos"] + ref["S_neg"]).sum().reshape(1), TAU)
    check(case, "ent.grad", grads[0], before[0], ref["grad_ent"], ref["S_ent"], TAU, ref["U_ent"], drop_level(ref, "ent"))
    check(case, "rel.grad", grads[1], before[1], ref["grad_rel"], ref["S_rel"], TAU, ref["U_rel"], drop_level(ref, "rel"))
    if P is not None:
        check(case, "proj.grad", grads[2], before[2], ref["grad_proj"], ref["S_proj"], TAU_DP_LONG if 2 * B >= 8192 else TAU, ref["U_proj"])
    return m, ref


# ---------------------------------------------------------------------------------------------------- a. shape sweep, MARGIN
SWEEP = [  # kind, norm, D, B, n_ent, n_rel: ragged N tiles / partial k steps (68, 100), 4 lane iterations (260 -> 2 for 260,
    # 768 -> 3, 1024 -> 4), gy = 2 and a 4-wide last tile (1028); B = 5 leaves 15 of 16 dP splits empty, B = 129 a 4-row last piece
    ("pkgm", "L2", 4, 1, 3, 1),
    ("pkgm", "L1", 68, 5, 7, 2),
    ("transe", "L2", 100, 37, 40, 3),
    ("pkgm", "L2", 100, 129, 60, 4),
    ("transe", "L1", 260, 129, 200, 5),
    ("pkgm", "L1", 260, 37, 50, 2),
    ("pkgm", "L2", 768, 129, 100, 3),
    ("transe", "L2", 768, 5, 9, 1),
    ("pkgm", "L2", 1024, 4096, 3000, 7),
    ("transe", "L1", 1024, 1, 2, 1),
    ("pkgm", "L1", 1028, 37, 30, 3),
    ("transe", "L2", 1028, 129, 100, 2),
    ("pkgm", "L2", 1028, 5, 11, 2),
]


@pytest.mark.parametrize("kind,norm,D,B,n_ent,n_rel", SWEEP, ids=[f"{k}-{n}-D{d}-B{b}" for k, n, d, b, _, _ in SWEEP])
def test_margin_step_shape_sweep(gpu, kind, norm, D, B, n_ent, n_rel):
    margin_case(f"sweep-{kind}-{norm}-D{D}-B{B}", kind, norm, D, B, n_ent, n_rel, gpu, seed=D * 7919 + B)


# ---------------------------------------------------------------------------------------------------- b. segment-sum structure
def designed_ids(counts, B, n_rel_keys, dev, seed):
    """4B entity ids with the given per-key counts (sorted positions follow from them), shuffled into h / nh / t / nt; then
    self-loops (t = h) and negatives equal to their positive (nh = h) by swaps inside one block, which keep the counts."""
    rs = np.random.RandomState(seed)
    keys = np.concatenate([np.full(c, k, np.int64) for k, c in counts])
    assert keys.size == 4 * B
    keys = rs.permutation(keys)
    h, nh, t, nt = (keys[i * B:(i + 1) * B].copy() for i in range(4))

    def pull(block, i, value):
        j = np.flatnonzero(block == value)
        j = j[j != i]
        if j.size:
            block[i], block[j[0]] = block[j[0]], block[i]

    for i in range(0, B, 7):
        pull(t, i, h[i])                    # self-loop
    for i in range(3, B, 11):
        pull(nh, i, h[i])                   # negative head equal to the positive head
    r = rs.randint(0, n_rel_keys, B).astype(np.int64)
    return [torch.from_numpy(x).to(dev) for x in (h, t, r, nh, nt)]


def test_segment_sums_over_designed_runs(gpu):
    B, D = 1029, 260                                        # M = 4116 entity rows: 8 full pieces and a 20-row last one
    # sorted positions: key 0 -> [0, 512) ends on a boundary; key 1 -> [512, 1024) starts and ends on one; key 2 starts at 1024;
    # key 3 -> [1029, 3129) covers pieces 3, 4 and 5 whole; then short runs up to the last piece
    counts = [(0, 512), (1, 512), (2, 5), (3, 2100)]
    rest = 4 * B - sum(c for _, c in counts)
    k = 4
    while rest:
        c = min(rest, 1 + (k % 3))
        counts.append((k, c))
        rest -= c
        k += 1
    n_ent = k + 5                                           # 5 rows nobody touches
    ids = designed_ids(counts, B, 1, gpu, seed=5)           # every fact on relation 0: its run is all 5 relation pieces
    h, t, r, nh, nt = ids
    assert (h == t).sum() > 0 and (nh == h).sum() > 0
    order = torch.argsort(torch.cat([h, nh, t, nt]), stable=True)
    keys = torch.cat([h, nh, t, nt])[order].cpu()
    assert keys[511] == 0 and keys[512] == 1 and keys[1023] == 1 and keys[1024] == 2 and (keys[1536:3072] == 3).all()
    for kind, norm in (("pkgm", "L2"), ("transe", "L1")):
        m, ref = margin_case(f"seg-{kind}-{norm}", kind, norm, D, B, n_ent, 3, gpu, seed=17, ids=ids)
        assert (ref["count_rel"][1:] == 0).all() and ref["count_ent"][-5:].eq(0).all()


# ---------------------------------------------------------------------------------------------------- c. exact edges on a grid
def grid_case(kind, norm, k, B, n_ent, n_rel, seed, dev):
    """Entity rows +-2^-k with D = 4^k (unit norm: normalize is exact), relation entries in 2^-k * {-1, 0, 1}, P in
    2^-k * {-1, 0, 1}: every fp32 operation of the step is exact, so the kernel and fp64 take every sign and tie alike."""
    D = 4 ** k
    g = torch.Generator(device="cpu").manual_seed(seed)
    ent = (torch.randint(0, 2, (n_ent, D), generator=g) * 2 - 1).float() * 2.0 ** -k
    rel = (torch.randint(-1, 2, (n_rel, D), generator=g)).float() * 2.0 ** -k
    P = (torch.randint(-1, 2, (D, D), generator=g)).float() * 2.0 ** -k if kind == "pkgm" else None
    ids = rand_ids(B, n_ent, n_rel, dev, seed + 1)
    return D, ent.to(dev), rel.to(dev), None if P is None else P.to(dev), ids


@pytest.mark.parametrize("kind,norm,k", [("pkgm", "L1", 2), ("transe", "L1", 3), ("pkgm", "L2", 3)])
def test_exact_grid_signs_and_hinge_tie(gpu, kind, norm, k):
    B, n_ent, n_rel = 300, 40, 3
    nrm = 2 if norm == "L2" else 1
    D, ent, rel, P, ids = grid_case(kind, norm, k, B, n_ent, n_rel, seed=31 + k, dev=gpu)
    h, t, r, nh, nt = ids
    pos, neg = R.scores(ent, rel, P, *ids, nrm)
    # margin = pos - neg of one pair whose negative differs from its positive (a gradient that cannot cancel)
    cand = torch.nonzero(((nh != h) | (nt != t)) & (pos != neg)).flatten()
    i = int(cand[0])
    margin = (pos[i] - neg[i]).item()
    assert R.f32(margin) == margin and margin - pos[i].item() + neg[i].item() == 0.0
    ref = R.score_step(ent, rel, P, *ids, nrm, margin=margin)            # torch's margin_ranking_loss: active at the tie
    assert bool(ref["act"][i])
    heads, tails = torch.cat([h, nh]), torch.cat([t, nt])
    u = F64n(ent, heads) + rel.double()[torch.cat([r, r])] - F64n(ent, tails)
    assert (u == 0).sum() > 50                                           # many exact zero differences: sign(0) matters
    if P is not None:
        w = F64n(ent, heads) @ P.double().T - rel.double()[torch.cat([r, r])]
        assert (w == 0).sum() > 50
    m = make_model(kind, norm, ent, rel, P)
    runs = []
    for _ in range(2):
        set_grads(m, [torch.zeros_like(p) for p in m.tables()])
        loss, kp, kn = m.margin_step(*ids, margin=margin)
        torch.cuda.synchronize()
        runs.append([loss, kp, kn] + [p.grad.clone() for p in m.tables()])
    for a, b in zip(*runs):
        assert torch.equal(a, b), "a second identical call differs"
    assert torch.equal(kp.double(), ref["pos"]) and torch.equal(kn.double(), ref["neg"])
    assert loss.item() == ref["loss"].item()
    for p, key in zip(m.tables(), ("grad_ent", "grad_rel", "grad_proj")):
        assert torch.equal(p.grad.double(), ref[key]), key                # exact: every sign, the tie and every sum


def F64n(ent, idx):
    return torch.nn.functional.normalize(ent.double()[idx], p=2, dim=1)


def test_zero_entity_row_gets_dy_over_eps(gpu):
    """F.normalize of a zero row backpropagates dy / 1e-12; the kernel must do the same (its own case: the size swamps others)."""
    D, B = 68, 3
    ent, rel, P = rand_tables(6, 2, D, True, gpu, seed=41)
    ent[2] = 0
    ids = [torch.tensor(x, device=gpu) for x in ([2, 0, 1], [3, 4, 5], [0, 1, 0], [1, 2, 5], [4, 3, 2])]
    m, ref = margin_case("zero-row", "pkgm", "L2", D, B, 6, 2, gpu, seed=41, ids=ids, tabs=(ent, rel, P))
    g = ref["grad_ent"][2]
    assert g.abs().max().item() > 1e10                                   # the 1e12 scale is really there


# ---------------------------------------------------------------------------------------------------- d. modes and reuse
def test_score_mode_leaves_gradients_alone_and_grad_mode_takes_real_upstreams(gpu):
    D, B, n_ent, n_rel = 260, 129, 150, 4
    ent, rel, P = rand_tables(n_ent, n_rel, D, True, gpu, seed=51)
    ids = rand_ids(B, n_ent, n_rel, gpu, seed=52)
    m = make_model("pkgm", "L2", ent, rel, P)
    before = sentinel_grads(m, 53)
    set_grads(m, before)
    pos, neg = m(*ids)                                                   # SCORE mode
    torch.cuda.synchronize()
    for p, b in zip(m.tables(), before):
        assert torch.equal(p.grad, b)
    g = torch.Generator(device="cpu").manual_seed(54)
    wp, wn = torch.randn(B, generator=g).to(gpu), torch.randn(B, generator=g).to(gpu)
    for name, fn, dp, dn in (("both", lambda p, n: (wp * p).sum() + (wn * n).sum(), wp, wn),
                             ("pos-only", lambda p, n: (wp * p).sum(), wp, torch.zeros_like(wn)),
                             ("neg-only", lambda p, n: (wn * n).sum(), torch.zeros_like(wp), wn)):
        ref = R.score_step(ent, rel, P, *ids, 2, dpos=dp, dneg=dn)
        case = f"grad-mode-{name}"
        runs = []
        for _ in range(2):
            set_grads(m, before)
            pos, neg = m(*ids)
            fn(pos, neg).backward()                                     # GRAD mode through _KGScoreFn.backward
            torch.cuda.synchronize()
            runs.append([pos.detach().clone(), neg.detach().clone()] + [p.grad.clone() for p in m.tables()])
        for a, b in zip(*runs):
            assert torch.equal(a, b), f"{case}: a second identical call differs"
        pos, neg, *grads = runs[0]
        check(case, "pos", pos, torch.zeros_like(pos), ref["pos"], ref["S_pos"], TAU)
        check(case, "neg", neg, torch.zeros_like(neg), ref["neg"], ref["S_neg"], TAU)
        check(case, "ent.grad", grads[0], before[0], ref["grad_ent"], ref["S_ent"], TAU, None, drop_level(ref, "ent"))
        check(case, "rel.grad", grads[1], before[1], ref["grad_rel"], ref["S_rel"], TAU, None, drop_level(ref, "rel"))
        check(case, "proj.grad", grads[2], before[2], ref["grad_proj"], ref["S_proj"], TAU)


def test_workspace_reuse_large_then_short_batch(gpu):
    D, n_ent, n_rel = 768, 2000, 5
    tabs = rand_tables(n_ent, n_rel, D, True, gpu, seed=61)
    m, _ = margin_case("reuse-B4096", "pkgm", "L2", D, 4096, n_ent, n_rel, gpu, seed=61, tabs=tabs)
    ws = m._ws.data_ptr()
    margin_case("reuse-B37", "pkgm", "L2", D, 37, n_ent, n_rel, gpu, seed=62, m=m, tabs=tabs)
    assert m._ws.data_ptr() == ws                                        # the short batch ran in the large batch's workspace


# ---------------------------------------------------------------------------------------------------- e. out-of-range ids
def carve(x, pad):
    """x copied into the middle of a buffer with `pad` floats of random canary on each side: (view, whole buffer)."""
    buf = torch.randn(x.numel() + 2 * pad, device=x.device)
    view = buf[pad:pad + x.numel()].view(x.shape)
    view.copy_(x)
    return view, buf


def call_score(lib, ent, rel, P, ids, B, D, n_ent, n_rel, norm, mode, margin, dpos, dneg, pos, neg, loss, orders, grads, ws, nbytes):
    ptr = lambda x: None if x is None else x.data_ptr()  # noqa: E731
    return lib.ia_kgpt_score(ptr(ent), ptr(rel), ptr(P), *(ptr(x) for x in ids), B, D, n_ent, n_rel, norm, mode, float(margin), ptr(dpos),
                             ptr(dneg), ptr(pos), ptr(neg), ptr(loss), *(ptr(o) for o in orders), *(ptr(g) for g in grads), ptr(ws), nbytes,
                             stream_ptr())


def orders_of(ids):
    h, t, r, nh, nt = ids
    return tuple(torch.argsort(k, stable=True).to(torch.int32) for k in (torch.cat([h, nh, t, nt]), torch.cat([r, r])))


def test_out_of_range_ids_read_zero_rows_and_get_no_gradient(gpu):
    lib = _lib.load()
    D, B, n_ent, n_rel = 68, 37, 20, 3
    ent0, rel0, P0 = rand_tables(n_ent, n_rel, D, True, gpu, seed=71)
    h, t, r, nh, nt = rand_ids(B, n_ent, n_rel, gpu, seed=72)
    h[0], t[1], nh[2], nt[3], h[4], t[5], nh[6], nt[7] = -1, -1, -1, -1, n_ent, n_ent, n_ent, n_ent
    r[8], r[9] = -1, n_rel
    ids = [h, t, r, nh, nt]
    ent, ent_buf = carve(ent0, D)
    rel, rel_buf = carve(rel0, D)
    P, P_buf = carve(P0, D)
    g = torch.Generator(device="cpu").manual_seed(73)
    before = [(torch.randn(x.shape, generator=g) * 1e-2).to(gpu) for x in (ent0, rel0, P0)]
    carved = [carve(b, D) for b in before]
    snap = [b.clone() for b in (ent_buf, rel_buf, P_buf)] + [c[1].clone() for c in carved]
    margin = pick_margin(ent0, rel0, P0, ids, "L2")
    ref = R.score_step(ent0, rel0, P0, *ids, 2, margin=margin)
    nbytes = lib.ia_kgpt_workspace_bytes(B, D, 1)
    ws = torch.empty(nbytes, device=gpu, dtype=torch.uint8)
    runs = []
    for _ in range(2):
        for (view, _buf), b in zip(carved, before):
            view.copy_(b)
        pos, neg, loss = torch.empty(B, device=gpu), torch.empty(B, device=gpu), torch.empty(1, device=gpu)
        rc = call_score(lib, ent, rel, P, ids, B, D, n_ent, n_rel, 2, K.KGPT_MARGIN, margin, None, None, pos, neg, loss, orders_of(ids),
                        [c[0] for c in carved], ws, nbytes)
        torch.cuda.synchronize()
        assert rc == 0
        runs.append([pos, neg, loss] + [c[1].clone() for c in carved])
    for a, b in zip(*runs):
        assert torch.equal(a, b), "out-of-range: a second identical call differs"
    for (view, buf), whole in zip(carved, runs[0][3:]):
        buf.copy_(whole)                                                 # the first call's gradients, canaries included
    for buf, s in zip([ent_buf, rel_buf, P_buf] + [c[1] for c in carved], snap):
        assert torch.equal(buf[:D], s[:D]) and torch.equal(buf[-D:], s[-D:]), "a canary next to a table or gradient changed"
    assert torch.equal(ent_buf, snap[0]) and torch.equal(rel_buf, snap[1]) and torch.equal(P_buf, snap[2])
    case = "out-of-range"
    check(case, "pos", pos, torch.zeros_like(pos), ref["pos"], ref["S_pos"], TAU)
    check(case, "neg", neg, torch.zeros_like(neg), ref["neg"], ref["S_neg"], TAU)
    check(case, "ent.grad", carved[0][0], before[0], ref["grad_ent"], ref["S_ent"], TAU, None, drop_level(ref, "ent"))
    check(case, "rel.grad", carved[1][0], before[1], ref["grad_rel"], ref["S_rel"], TAU, None, drop_level(ref, "rel"))
    check(case, "proj.grad", carved[2][0], before[2], ref["grad_proj"], ref["S_proj"], TAU)


# ---------------------------------------------------------------------------------------------------- f. ABI refusals
def test_abi_refusals_do_not_launch(gpu):
    lib = _lib.load()
    D, B, n_ent, n_rel = 8, 4, 5, 2
    ent, rel, P = rand_tables(n_ent, n_rel, D, True, gpu, seed=81)
    ids = rand_ids(B, n_ent, n_rel, gpu, seed=82)
    orders = orders_of(ids)
    grads = [torch.zeros_like(x) for x in (ent, rel, P)]
    nbytes = lib.ia_kgpt_workspace_bytes(B, D, 1)
    ws = torch.empty(nbytes, device=gpu, dtype=torch.uint8)
    pos, neg, loss = (torch.full((n,), 7.0, device=gpu) for n in (B, B, 1))
    dz = torch.zeros(B, device=gpu)
    base = dict(ent=ent, rel=rel, P=P, ids=ids, B=B, D=D, n_ent=n_ent, n_rel=n_rel, norm=2, mode=K.KGPT_MARGIN, margin=1.0, dpos=None,
                dneg=None, pos=pos, neg=neg, loss=loss, orders=orders, grads=grads, ws=ws, nbytes=nbytes)
    bad = [("D % 4", dict(D=6), _lib_err("ARG")), ("B = 0", dict(B=0), _lib_err("ARG")), ("B < 0", dict(B=-3), _lib_err("ARG")),
           ("norm 0", dict(norm=0), _lib_err("ARG")), ("norm 3", dict(norm=3), _lib_err("ARG")),
           ("mode -1", dict(mode=-1), _lib_err("ARG")), ("mode 3", dict(mode=3), _lib_err("ARG")),
           ("GRAD without dpos", dict(mode=K.KGPT_GRAD, dneg=dz), _lib_err("ARG")),
           ("GRAD without orders", dict(mode=K.KGPT_GRAD, dpos=dz, dneg=dz, orders=(None, None)), _lib_err("ARG")),
           ("MARGIN without orders", dict(orders=(None, orders[1])), _lib_err("ARG")),
           ("workspace one byte short", dict(nbytes=nbytes - 1), _lib_err("WORKSPACE"))]
    for what, over, want in bad:
        a = dict(base, **over)
        rc = call_score(lib, a["ent"], a["rel"], a["P"], a["ids"], a["B"], a["D"], a["n_ent"], a["n_rel"], a["norm"], a["mode"], a["margin"],
                        a["dpos"], a["dneg"], a["pos"], a["neg"], a["loss"], a["orders"], a["grads"], a["ws"], a["nbytes"])
        torch.cuda.synchronize()
        assert rc == want, (what, rc)
        assert (pos == 7).all() and (neg == 7).all() and (loss == 7).all(), f"{what}: refused but launched"
        assert all((x == 0).all() for x in grads), what


def _lib_err(name):
    """IA_ERR_<name> as include/itemalign.h defines it."""
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "itemalign.h")).read()
    return int(re.search(rf"#define IA_ERR_{name} \((-?\d+)\)", header).group(1))


# ---------------------------------------------------------------------------------------------------- g. Adam
TAU_ADAM = 1e-6


@pytest.mark.parametrize("n", [1, 2, 3, 5, 4099, 8_388_620])
def test_adam_l2_against_fp64(gpu, n):
    lib = _lib.load()
    steps = 10
    lrs = [R.f32(1e-2 * (1 + 0.37 * i) * (0.5 if i % 3 == 0 else 1.0)) for i in range(steps)]
    g = torch.Generator(device=gpu).manual_seed(n)
    p0 = torch.randn(n, device=gpu, generator=g)
    grads = [torch.randn(n, device=gpu, generator=g) * (1 + i) for i in range(steps)]
    pad = 8
    for wd in (0.0, 1e-5, 1e-2):
        bufs = [torch.randn(n + pad, device=gpu, generator=g) for _ in range(4)]      # p, grad, m, v with a canary after element n
        p, gr, m, v = (b[:n] for b in bufs)
        p.copy_(p0)
        m.zero_()
        v.zero_()
        canary = [b[n:].clone() for b in bufs]
        for step, (gs, lr) in enumerate(zip(grads, lrs), 1):
            gr.copy_(gs)
            assert lib.ia_kgpt_adam_l2(p.data_ptr(), gr.data_ptr(), m.data_ptr(), v.data_ptr(), n, lr, 0.9, 0.999, 1e-8, wd, step,
                                       stream_ptr()) == 0
            torch.cuda.synchronize()
            assert (gr == 0).all(), "the gradient is not cleared"
        for b, c in zip(bufs, canary):
            assert torch.equal(b[n:], c), "a canary after element n changed"
        # the C ABI takes fp32 betas / eps: the reference runs with exactly those values
        rp, rm, rv, Sp, Sm, Sv = R.adam_l2(p0, torch.zeros(n, device=gpu), torch.zeros(n, device=gpu), grads, lrs, beta1=R.f32(0.9),
                                           beta2=R.f32(0.999), eps=R.f32(1e-8), weight_decay=wd)
        # yardstick: torch's own fp32 Adam (single-tensor path)
        tp = torch.nn.Parameter(p0.clone())
        opt = torch.optim.Adam([tp], lr=lrs[0], weight_decay=wd, foreach=False)
        for gs, lr in zip(grads, lrs):
            opt.param_groups[0]["lr"] = lr
            tp.grad = gs.clone()
            opt.step()
        case = f"adam-n{n}-wd{wd:g}"
        zero = torch.zeros_like(p)
        qp = check(case, "param", p, zero, rp, Sp, TAU_ADAM)
        check(case, "exp_avg", m, zero, rm, Sm, TAU_ADAM)
        check(case, "exp_avg_sq", v, zero, rv, Sv, TAU_ADAM)
        qt = ((tp.detach().double() - rp).abs() / Sp).max().item()
        print(f"KGPT-BOUND {case} torch-fp32-Adam param max|err|/S={qt:.3e}")
        assert qp <= 4 * qt + 4 * EPS32, (qp, qt)


def test_adam_l2_refuses_misaligned_pointers(gpu):
    lib = _lib.load()
    buf = torch.zeros(4, 12, device=gpu)
    ptrs = [b.data_ptr() for b in buf]
    for i in range(4):
        bad = list(ptrs)
        bad[i] += 4
        assert lib.ia_kgpt_adam_l2(*bad, 7, 1e-3, 0.9, 0.999, 1e-8, 0.0, 1, stream_ptr()) == -1
    torch.cuda.synchronize()
    assert (buf == 0).all()


# ---------------------------------------------------------------------------------------------------- h. row normalise
@pytest.mark.parametrize("D", [4, 260, 768, 1028])
def test_row_normalize_against_fp64(gpu, D):
    lib = _lib.load()
    rows = 37
    g = torch.Generator(device=gpu).manual_seed(D)
    scale = torch.tensor([10.0 ** e for e in (-15, -6, 0, 6, 15)], device=gpu).repeat(8)[:rows, None]
    x0 = torch.randn(rows, D, device=gpu, generator=g) * scale
    x0[3] = 0
    buf = torch.randn(rows * D + 2 * D, device=gpu, generator=g)
    x = buf[D:D + rows * D].view(rows, D)
    x.copy_(x0)
    snap = buf.clone()
    assert lib.ia_kgpt_row_normalize(x.data_ptr(), rows, D, stream_ptr()) == 0
    torch.cuda.synchronize()
    assert torch.equal(buf[:D], snap[:D]) and torch.equal(buf[-D:], snap[-D:]), "a canary next to the rows changed"
    assert (x[3] == 0).all()
    ref = R.row_normalize(x0)
    S = x0.double().abs() / x0.double().norm(dim=1, keepdim=True).clamp_min(R.NORM_EPS)
    check(f"row-normalize-D{D}", "x", x, torch.zeros_like(x), ref, S, TAU)


# ---------------------------------------------------------------------------------------------------- i. full size against fp64
def test_full_size_step_against_fp64_on_device(gpu):
    n_ent, n_rel, D, B = 258211, 1379, 1024, 32768
    g = torch.Generator(device=gpu).manual_seed(91)
    ent = torch.randn(n_ent, D, device=gpu, generator=g) * torch.exp(torch.randn(n_ent, 1, device=gpu, generator=g))
    rel = torch.randn(n_rel, D, device=gpu, generator=g) / math.sqrt(D)
    P = torch.randn(D, D, device=gpu, generator=g) / math.sqrt(D)
    ids = [torch.randint(0, n, (B,), device=gpu, generator=g) for n in (n_ent, n_ent, n_rel, n_ent, n_ent)]
    m = make_model("pkgm", "L2", ent, rel, P)
    before = sentinel_grads(m, 92)
    set_grads(m, before)
    with torch.no_grad():
        p0, n0 = m(*ids)                                                 # SCORE mode: a margin with about half of the pairs active
    margin = R.f32((p0 - n0).median().item())
    loss, pos, neg = m.margin_step(*ids, margin=margin)
    assert torch.equal(pos, p0) and torch.equal(neg, n0)
    torch.cuda.synchronize()
    grads = [p.grad.clone() for p in m.tables()]
    set_grads(m, before)
    loss2, pos2, neg2 = m.margin_step(*ids, margin=margin)
    torch.cuda.synchronize()
    assert torch.equal(loss, loss2) and torch.equal(pos, pos2) and torch.equal(neg, neg2)
    assert all(torch.equal(a, p.grad) for a, p in zip(grads, m.tables()))
    del loss2, pos2, neg2
    m.ent_emb.weight.grad = m.rel_emb.weight.grad = m.proj_mat.weight.grad = None
    # the kernel's own hinge decisions, recomputed bit-exactly in fp32 from its pos / neg
    act = (torch.tensor(margin, device=gpu) - pos + neg) >= 0
    assert 0.1 < act.double().mean().item() < 0.9
    ref = R.score_step(ent, rel, P, *ids, 2, margin=margin, active=act)
    case = "full-size"
    check(case, "pos", pos, torch.zeros_like(pos), ref["pos"], ref["S_pos"], TAU)
    check(case, "neg", neg, torch.zeros_like(neg), ref["neg"], ref["S_neg"], TAU)
    check(case, "loss", loss, torch.zeros_like(loss), ref["loss"].reshape(1), (ref["S_pos"] + ref["S_neg"]).sum().reshape(1), TAU)
    check(case, "ent.grad", grads[0], before[0], ref["grad_ent"], ref["S_ent"], TAU, None, drop_level(ref, "ent"))
    check(case, "rel.grad", grads[1], before[1], ref["grad_rel"], ref["S_rel"], TAU, None, drop_level(ref, "rel"))
    check(case, "proj.grad", grads[2], before[2], ref["grad_proj"], ref["S_proj"], TAU_DP_LONG)
