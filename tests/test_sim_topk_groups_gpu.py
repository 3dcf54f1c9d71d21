"""The grouped similarity top-k kernels (ia_sim_topk_groups, ia_sim_topk_fold, ia_sim_centroid_sums; csrc/simtopk_groups.hip) against
tests/ivf_reference.py.

On exact operands (whole numbers in [-4, 4], D <= 200: every partial sum is a whole number below 2^24, so the fp32 accumulation is exact
in any order) ids and scores are compared bit for bit with the fp64 selection per group: twelve groups in one call whose candidate counts
sit on the edges of the 128-candidate tile and whose query counts sit on the edges of the 32-query wave and of the 128 / 256-query tile,
the groups without queries and without candidates among them, with and without skipped positions and labels, for every cap on the
candidate ranges and with the groups stored in another order.  The matrices are surrounded by NaN rows, and the rows the layout lets
nobody read (the queries of a group without candidates, the candidates of a group without queries) are NaN too: a tail tile that
reached into a neighbour would bring a NaN into a list.  On random rows the lists have to pass check_topk with the accumulator bar,
and one group covering everything has to give the bits of ia_sim_topk."""
import numpy as np
import pytest
import torch

import ivf_reference as IR
import simtopk_reference as SR

pytestmark = pytest.mark.gpu

BF16, F32 = torch.bfloat16, torch.float32
N_CAND = (0, 1, 5, 127, 128, 129, 257, 129, 5, 257, 128, 1)   # group 0: queries without candidates
N_QUERY = (33, 0, 1, 31, 33, 127, 128, 129, 257, 0, 257, 129)  # groups 1 and 9: candidates without queries
PAD = 3                                                       # NaN rows in front of the first group and behind the last


def _R():
    from item_alignment_amd import retrieval
    return retrieval


def _ints(seed, n, D, pool=None):
    g = torch.Generator().manual_seed(seed)
    if pool is None:
        return torch.randint(-4, 5, (n, D), generator=g).to(F32)
    return torch.randint(-4, 5, (pool, D), generator=g).to(F32)[torch.randint(0, pool, (n,), generator=g)]


def _layout(qg, cg, order, dev):
    """The groups' rows (lists of fp32 matrices) stored in `order` between NaN rows.  -> q, c: fp32 [rows, D] with NaN where nothing
    may be read; their prepared bf16 copies on the device; q_off, c_off int64 [G + 1]; the first row of every group in q and in c,
    indexed by the group's number (not its place)."""
    D = qg[0].shape[1]
    nan = torch.full((PAD, D), float("nan"))
    q_parts, c_parts, q_off, c_off = [nan], [nan], [PAD], [PAD]
    q_at, c_at = {}, {}
    for g in order:
        q_at[g], c_at[g] = q_off[-1], c_off[-1]
        q_parts.append(qg[g] if len(cg[g]) else torch.full_like(qg[g], float("nan")))
        c_parts.append(cg[g] if len(qg[g]) else torch.full_like(cg[g], float("nan")))
        q_off.append(q_off[-1] + len(qg[g]))
        c_off.append(c_off[-1] + len(cg[g]))
    q, c = torch.cat(q_parts + [nan]), torch.cat(c_parts + [nan])
    pitch = _R().row_pitch(D)

    def prepared(x):
        out = torch.full((x.shape[0], pitch), float("nan"), dtype=BF16)    # the pad columns of a NaN row are NaN too
        out[~torch.isnan(x[:, 0])] = 0
        out[:, :D] = x.to(BF16)
        return out.to(dev)
    return q, c, prepared(q), prepared(c), np.array(q_off), np.array(c_off), q_at, c_at


def _bits_equal(idx, score, want_idx, want_score, what):
    idx, score = idx.cpu().numpy(), score.cpu().numpy()
    assert not np.isnan(score).any(), (what, "a NaN reached a list")
    assert np.array_equal(idx, want_idx), (what, "ids", np.argwhere(idx != want_idx)[:4])
    assert np.array_equal(score.view(np.int32), want_score.view(np.int32)), (what, "scores", np.argwhere(score != want_score)[:4])


def _skips(q_off, c_off, q_rows):
    """a position per query row: of its own group mostly, none for every fifth row, of the NEXT group's range (skips nothing) for every
    seventh"""
    skip = np.full(q_rows, -1, np.int64)
    for g in range(len(q_off) - 1):
        n = c_off[g + 1] - c_off[g]
        for p in range(q_off[g], q_off[g + 1]):
            if p % 7 == 6:
                skip[p] = c_off[g + 1] + 2
            elif p % 5 != 4 and n:
                skip[p] = c_off[g] + (p * 7) % n
    return skip


# ------------------------------------------------------------------------------------------------ exact operands
@pytest.mark.parametrize("k", [1, 10, 64])
@pytest.mark.parametrize("D", [8, 72, 200])
def test_exact_operands_bit_equal(gpu, D, k):
    R = _R()
    G = len(N_CAND)
    qg = [_ints(100 + g, N_QUERY[g], D) for g in range(G)]
    cg = [_ints(200 + g, N_CAND[g], D, pool=40) for g in range(G)]      # duplicates inside a group: ties between reported ids
    q, c, qd, cd, q_off, c_off, q_at, c_at = _layout(qg, cg, list(range(G)), gpu)
    rev = torch.arange(c.shape[0] - 1, -1, -1)                          # label: a reversed permutation of the positions
    skip = _skips(q_off, c_off, q.shape[0])
    base = {}
    for label in (None, rev):
        for sk in (None, skip):
            want = IR.select_groups(q, c, q_off, c_off, k, label=label, skip=sk)
            for ms in (0, 1, 2):
                got = R.sim_topk_groups(qd, cd, q_off, c_off, D, k, label=None if label is None else label.to(gpu), skip=sk, max_splits=ms)
                _bits_equal(*got, *want, (D, k, label is not None, sk is not None, ms))
            lab32 = R.sim_topk_groups(qd, cd, q_off, c_off, D, k, label=None if label is None else label.to(gpu, torch.int32), skip=sk)
            _bits_equal(*lab32, *want, (D, k, "int32 labels", sk is not None))
            base[(label is not None, sk is not None)] = want
    # the same groups stored in another order, identified by their labels: the same lists for every query row
    order = [7, 2, 11, 0, 5, 9, 3, 10, 1, 8, 6, 4]
    q2, c2, qd2, cd2, q_off2, c_off2, q_at2, c_at2 = _layout(qg, cg, order, gpu)
    label2 = torch.full((c2.shape[0],), 0, dtype=torch.int64)
    skip2 = np.full(q2.shape[0], -1, np.int64)
    for g in range(G):
        label2[c_at2[g]:c_at2[g] + N_CAND[g]] = rev[c_at[g]:c_at[g] + N_CAND[g]]
        s = skip[q_at[g]:q_at[g] + N_QUERY[g]]
        inside = (s >= c_at[g]) & (s < c_at[g] + N_CAND[g])
        skip2[q_at2[g]:q_at2[g] + N_QUERY[g]] = np.where(inside, s - c_at[g] + c_at2[g], -1)
    idx2, sc2 = (t.cpu().numpy() for t in R.sim_topk_groups(qd2, cd2, q_off2, c_off2, D, k, label=label2.to(gpu), skip=skip2))
    want = base[(True, True)]
    for g in range(G):
        a, b = slice(q_at2[g], q_at2[g] + N_QUERY[g]), slice(q_at[g], q_at[g] + N_QUERY[g])
        assert np.array_equal(idx2[a], want[0][b]) and np.array_equal(sc2[a].view(np.int32), want[1][b].view(np.int32)), ("reordered", g)


@pytest.mark.parametrize("k", [10, 64])
def test_duplicates_in_different_groups_come_out_by_label_through_the_fold(gpu, k):
    """a catalogue of 600 rows drawn from 50 distinct ones, cut into 6 lists by a random assignment and stored list by list; 70 queries
    probe 3 lists each.  scan + fold against the exact selection over the probed lists, in (score descending, original row ascending)"""
    R = _R()
    N, D, nlist, nprobe, B = 600, 72, 6, 3, 70
    x = _ints(7, N, D, pool=50)
    g = torch.Generator().manual_seed(8)
    assignment = torch.randint(0, nlist, (N,), generator=g)
    row_id = assignment.argsort(stable=True)
    inv = torch.empty_like(row_id)
    inv[row_id] = torch.arange(N)
    c_off = np.concatenate([[0], np.cumsum(np.bincount(assignment.numpy(), minlength=nlist))])
    queries = x[:B]                                            # catalogue rows 0 .. B - 1, each kept out of its own list
    probes = torch.stack([torch.randperm(nlist, generator=g)[:nprobe] for _ in range(B)])
    flat = probes.reshape(-1)
    order = flat.argsort(stable=True)
    src = order // nprobe
    rows_of = torch.empty_like(order)
    rows_of[order] = torch.arange(order.numel())
    q_off = np.concatenate([[0], np.cumsum(np.bincount(flat.numpy(), minlength=nlist))])
    pitch = R.row_pitch(D)

    def prepared(m):
        out = torch.zeros(m.shape[0], pitch, dtype=BF16)
        out[:, :D] = m.to(BF16)
        return out.to(gpu)
    gi, gs = R.sim_topk_groups(prepared(queries[src]), prepared(x[row_id]), q_off, c_off, D, k, label=row_id.to(gpu), skip=inv[src])
    got = R.sim_topk_fold(gi, gs, rows_of.view(B, nprobe).to(gpu))
    scores = SR.scores_fp64(queries, x).astype(np.float32)
    _bits_equal(*got, *IR.select_probed(scores, assignment, probes, k, skip=np.arange(B)), ("fold", k))
    # a query without lists, and one with a single list
    rows_of2 = rows_of.view(B, nprobe).clone()
    rows_of2[0] = -1
    rows_of2[1, 1:] = -1
    i2, s2 = (t.cpu() for t in R.sim_topk_fold(gi, gs, rows_of2.to(gpu)))
    assert (i2[0] == -1).all() and torch.isneginf(s2[0]).all()
    assert torch.equal(i2[1], gi[rows_of2[1, 0]].cpu()) and torch.equal(s2[1], gs[rows_of2[1, 0]].cpu())
    assert torch.equal(i2[2:], got[0][2:].cpu())


# ------------------------------------------------------------------------------------------------ random rows
@pytest.mark.parametrize("k", [10, 64])
def test_random_rows_within_the_bar_per_group(gpu, k):
    R = _R()
    D, nc, nq = 200, (129, 40, 300, 5), (130, 257, 33, 64)
    g = torch.Generator().manual_seed(k)

    def unit(n):
        return torch.nn.functional.normalize(torch.randn(n, D, generator=g), dim=1).to(BF16).to(F32)
    qg, cg = [unit(n) for n in nq], [unit(n) for n in nc]
    q, c, qd, cd, q_off, c_off, q_at, c_at = _layout(qg, cg, [0, 1, 2, 3], gpu)
    skip = _skips(q_off, c_off, q.shape[0])
    idx, score = (t.cpu().numpy() for t in R.sim_topk_groups(qd, cd, q_off, c_off, D, k, skip=skip))
    again = R.sim_topk_groups(qd, cd, q_off, c_off, D, k, skip=skip, max_splits=1)
    _bits_equal(*again, idx, score, "another cap on the ranges")
    assert (idx[:PAD] == -1).all() and (idx[-PAD:] == -1).all()
    for gr in range(4):
        rows = slice(q_at[gr], q_at[gr] + nq[gr])
        local = np.where(idx[rows] >= 0, idx[rows] - c_at[gr], -1)
        sk = np.where(skip[rows] >= 0, skip[rows] - c_at[gr], -1)      # a position of the next group falls outside [0, n): skips nothing
        SR.check_topk(local, score[rows], SR.scores_fp64(qg[gr], cg[gr]), SR.bar(qg[gr], cg[gr], R.row_pitch(D)), k, sk)


@pytest.mark.parametrize("k", [10, 64])
def test_one_group_covering_everything_is_sim_topk(gpu, k):
    R = _R()
    D, B, n = 72, 130, 1000
    g = torch.Generator().manual_seed(11)
    q = torch.nn.functional.normalize(torch.randn(B, D, generator=g), dim=1)
    c = torch.nn.functional.normalize(torch.randn(n, D, generator=g), dim=1)
    qd, cd = R.prepare_rows(q.to(gpu), False), R.prepare_rows(c.to(gpu), False)
    skip = (np.arange(B) * 7) % n
    want = R.sim_topk(qd, cd, D, k, skip=skip)
    for ms in (0, 1):
        got = R.sim_topk_groups(qd, cd, [0, B], [0, n], D, k, skip=skip, max_splits=ms)
        assert torch.equal(got[0], want[0]) and torch.equal(got[1].view(torch.int32), want[1].view(torch.int32)), (k, ms)


# ------------------------------------------------------------------------------------------------ buffers and edges
def test_nothing_outside_the_buffers_is_read_or_written(gpu):
    from item_alignment_amd import _lib
    R = _R()
    lib = _lib.load()
    D, k, GUARD = 72, 10, 4096
    pitch = R.row_pitch(D)
    qg, cg = [_ints(1, 130, D), _ints(2, 5, D)], [_ints(3, 257, D), _ints(4, 129, D)]
    q, c, qd, cd, q_off, c_off, _, _ = _layout(qg, cg, [0, 1], gpu)
    want = IR.select_groups(q, c, q_off, c_off, k)
    P, n = q.shape[0], c.shape[0]
    ops = torch.full((GUARD + P * pitch + GUARD + n * pitch + GUARD,), float("nan"), device=gpu, dtype=BF16)
    ops[GUARD:GUARD + P * pitch].view(P, pitch).copy_(qd)
    ops[2 * GUARD + P * pitch:2 * GUARD + (P + n) * pitch].view(n, pitch).copy_(cd)
    idx_buf = torch.full((GUARD + P * k + GUARD,), -777, device=gpu, dtype=torch.int64)
    sc_buf = torch.full((GUARD + P * k + GUARD,), 12345.0, device=gpu, dtype=F32)
    nbytes = lib.ia_sim_topk_groups_workspace_bytes(P, 2, D, n, k, 0)
    ws = torch.full((GUARD + nbytes + GUARD,), 0x5A, device=gpu, dtype=torch.uint8)
    offs = torch.full((64,), 1 << 40, device=gpu, dtype=torch.int64)      # q_off at [8:11], c_off at [24:27], huge values around them
    offs[8:11], offs[24:27] = torch.as_tensor(q_off), torch.as_tensor(c_off)
    rc = lib.ia_sim_topk_groups(ops[GUARD:].data_ptr(), ops[2 * GUARD + P * pitch:].data_ptr(), offs[8:].data_ptr(), offs[24:].data_ptr(), 2, P, D,
                                n, None, 0, None, k, 0, idx_buf[GUARD:].data_ptr(), sc_buf[GUARD:].data_ptr(), ws[GUARD:].data_ptr(), nbytes,
                                _lib.stream_ptr())
    assert rc == 0
    torch.cuda.synchronize()
    got_idx, got_sc = idx_buf[GUARD:GUARD + P * k].view(P, k), sc_buf[GUARD:GUARD + P * k].view(P, k)
    inside = slice(PAD, P - PAD)                               # the rows of a group; the others are not written
    _bits_equal(got_idx[inside], got_sc[inside], want[0][inside], want[1][inside], "guarded")
    assert (got_idx[:PAD] == -777).all() and (got_idx[-PAD:] == -777).all() and (got_sc[:PAD] == 12345.0).all() and (got_sc[-PAD:] == 12345.0).all()
    for buf, fill in ((idx_buf, -777), (sc_buf, 12345.0), (ws, 0x5A)):
        assert (buf[:GUARD] == fill).all() and (buf[-GUARD:] == fill).all()


def test_empty_calls_and_argument_errors_leave_the_outputs_alone(gpu):
    from item_alignment_amd import _lib
    R = _R()
    lib = _lib.load()
    D, k = 8, 3
    qd, cd = R.prepare_rows(_ints(1, 5, D).to(gpu), False), R.prepare_rows(_ints(2, 9, D).to(gpu), False)
    off = torch.tensor([0, 5, 0, 9], device=gpu)              # q_off = off[0:2], c_off = off[2:4]
    idx = torch.full((5, k), -777, device=gpu, dtype=torch.int64)
    score = torch.full((5, k), 12345.0, device=gpu, dtype=F32)
    ws = torch.empty(1 << 16, device=gpu, dtype=torch.uint8)

    def call(G=1, P=5, n=9, k=k, w=ws.data_ptr(), wb=ws.numel(), q=qd.data_ptr()):
        rc = lib.ia_sim_topk_groups(q, cd.data_ptr(), off.data_ptr(), off[2:].data_ptr(), G, P, D, n, None, 0, None, k, 0, idx.data_ptr(),
                                    score.data_ptr(), w, wb, _lib.stream_ptr())
        torch.cuda.synchronize()
        return rc
    for bad in (dict(k=0), dict(k=65), dict(P=-1), dict(G=-1), dict(n=-1), dict(w=None), dict(wb=8), dict(q=qd.data_ptr() + 2)):
        assert call(**bad) == -1, bad
        assert (idx == -777).all() and (score == 12345.0).all(), bad
    assert call(G=0, w=None, wb=0) == 0 and call(P=0, w=None, wb=0) == 0
    assert (idx == -777).all() and (score == 12345.0).all()
    assert call(n=0) == 0                                      # no candidate rows at all: every slot unused
    assert (idx == -1).all() and torch.isneginf(score).all()
    assert call() == 0
    _bits_equal(idx, score, *SR.select(SR.scores_fp64(_ints(1, 5, D), _ints(2, 9, D)).astype(np.float32), k), "after the refusals")
    i0, s0 = R.sim_topk_groups(qd, cd, [0], [0], D, k)         # G == 0
    assert (i0 == -1).all() and torch.isneginf(s0).all() and i0.shape == (5, k)
    with pytest.raises(ValueError):
        R.sim_topk_groups(qd, cd, [0, 5], [0, 9], D, 65)
    with pytest.raises(ValueError):
        R.sim_topk_groups(qd, cd, [0, 5], [0, 5, 9], D, k)


# ------------------------------------------------------------------------------------------------ ia_sim_centroid_sums
def _lists(n, nlist, seed):
    """an assignment with list 2 empty -> (assignment, order, list_off)"""
    g = torch.Generator().manual_seed(seed)
    a = torch.randint(0, nlist - 1, (n,), generator=g)
    a = torch.where(a >= 2, a + 1, a)
    return a, a.argsort(stable=True), torch.cat([torch.zeros(1, dtype=torch.int64), torch.bincount(a, minlength=nlist).cumsum(0)])


@pytest.mark.parametrize("D", [8, 72, 300])
def test_centroid_sums_exact_operands(gpu, D):
    R = _R()
    n, nlist = 1000, 9
    x = _ints(D, n, D)
    a, order, off = _lists(n, nlist, 1)
    rows = R.prepare_rows(x.to(gpu), False)
    sums, counts = R.centroid_sums(rows, D, order.to(gpu), off.to(gpu))
    want, want_n = IR.lloyd_sums_fp64(x, a, nlist)
    assert np.array_equal(counts.cpu().numpy(), want_n) and want_n[2] == 0
    assert np.array_equal(sums.cpu().numpy().view(np.int32), want.astype(np.float32).view(np.int32))
    assert (sums[2].view(torch.int32) == 0).all(), "an empty list gives zeros"


def test_centroid_sums_random_rows_within_the_bound_and_reproducible(gpu):
    R = _R()
    n, nlist, D = 3000, 9, 200
    g = torch.Generator().manual_seed(2)
    rows = R.prepare_rows(torch.randn(n, D, generator=g).to(gpu), True)
    x = rows[:, :D].cpu().to(torch.float64)                    # the bf16 rows as exact numbers
    a, order, off = _lists(n, nlist, 3)
    sums, counts = R.centroid_sums(rows, D, order.to(gpu), off.to(gpu))
    want, want_n = IR.lloyd_sums_fp64(x, a, nlist)
    assert np.array_equal(counts.cpu().numpy(), want_n)
    mass, _ = IR.lloyd_sums_fp64(x.abs(), a, nlist)
    err = np.abs(sums.cpu().numpy().astype(np.float64) - want)
    bound = want_n[:, None] * 2.0 ** -23 * mass                # n - 1 adds, each within 2^-24 of a partial sum that is at most the mass
    assert (err <= bound).all(), (err.max(), np.argwhere(err > bound)[:4])
    again = R.centroid_sums(rows, D, order.to(gpu), off.to(gpu))
    assert torch.equal(again[0].view(torch.int32), sums.view(torch.int32)) and torch.equal(again[1], counts)
    # entries of order outside the rows are left out, and not counted
    bad = order.clone()
    bad[0], bad[1] = -1, n
    s2, c2 = R.centroid_sums(rows, D, bad.to(gpu), off.to(gpu))
    assert int(c2.sum()) == n - 2 and torch.isfinite(s2).all()
