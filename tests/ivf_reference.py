"""References of the inverted-file index (ia_sim_topk_groups, ia_sim_topk_fold, ia_sim_centroid_sums; csrc/simtopk_groups.hip;
retrieval.IVFItemIndex).  Host only: numpy and torch fp64, on top of tests/simtopk_reference.py.

* select_groups:   simtopk_reference.select applied per group, in the order (score descending, REPORTED id ascending): the reported
                   id of candidate position c is label[c] (c without labels); skip[p] is a candidate POSITION.
* select_probed:   the exact top-k of each query restricted to the union of its probed lists, in (score descending, original row
                   ascending); skip[b] is an ORIGINAL row.
* lloyd_sums_fp64: the sum of each list's rows in fp64 and the list lengths.
* check_layout:    the lists partition 0 .. N - 1, rows ascend inside a list, the offsets and the inverse are consistent.
* model_ivf:       the scan of the probed lists + the fold restated on the host, with four switches that inject the faults the
                   comparison with select_probed has to catch.
"""
import numpy as np
import torch

import simtopk_reference as SR


def _np(x, dtype=None):
    a = np.asarray(torch.as_tensor(x).detach().cpu().numpy())
    return a if dtype is None else a.astype(dtype)


def select_groups(q, c, q_off, c_off, k, label=None, skip=None):
    """(idx int64 [P, k], score fp32 [P, k]) numpy.  q [P, D], c [n, D]: the rows as exact numbers; q_off, c_off [G + 1].  Rows of q
    outside every group keep -1 / -inf."""
    q_off, c_off = _np(q_off, np.int64), _np(c_off, np.int64)
    P = q.shape[0]
    idx = np.full((P, k), -1, np.int64)
    sc = np.full((P, k), -np.inf, np.float32)
    for g in range(len(q_off) - 1):
        ql, qh, cl, ch = int(q_off[g]), int(q_off[g + 1]), int(c_off[g]), int(c_off[g + 1])
        if qh <= ql or ch <= cl:
            continue
        pos = np.arange(cl, ch)
        ids = pos if label is None else _np(label, np.int64)[pos]
        by_id = np.argsort(ids, kind="stable")                # the group's columns in ascending reported id: select breaks ties by column
        s = SR.scores_fp64(q[ql:qh], c[cl:ch][by_id]).astype(np.float32)
        sk = None
        if skip is not None:
            col_of = {int(p): col for col, p in enumerate(pos[by_id])}
            sk = np.array([col_of.get(int(skip[p]), -1) for p in range(ql, qh)], np.int64)
        i, v = SR.select(s, k, sk)
        idx[ql:qh] = np.where(i >= 0, ids[by_id][np.clip(i, 0, None)], -1)
        sc[ql:qh] = v
    return idx, sc


def select_probed(scores, assignment, probes, k, skip=None):
    """scores [B, N] in original row order; assignment [N]: the list of each row; probes [B, nprobe] (-1: none)."""
    scores, assignment, probes = np.asarray(scores), _np(assignment, np.int64), _np(probes, np.int64)
    B, N = scores.shape
    idx = np.full((B, k), -1, np.int64)
    sc = np.full((B, k), -np.inf, np.float32)
    for b in range(B):
        ids = np.nonzero(np.isin(assignment, probes[b][probes[b] >= 0]))[0]
        if skip is not None:
            ids = ids[ids != int(skip[b])]
        s = scores[b, ids]
        order = np.lexsort((ids, -s))[:k]
        idx[b, :len(order)] = ids[order]
        sc[b, :len(order)] = s[order]
    return idx, sc


def lloyd_sums_fp64(rows, assignment, nlist):
    """(sums fp64 [nlist, D], counts int64 [nlist]) numpy"""
    rows, assignment = _np(torch.as_tensor(rows).to(torch.float64)), _np(assignment, np.int64)
    sums = np.zeros((nlist, rows.shape[1]), np.float64)
    np.add.at(sums, assignment, rows)
    return sums, np.bincount(assignment, minlength=nlist).astype(np.int64)


def check_layout(row_id, inv, list_off, assignment):
    row_id, inv, list_off, assignment = (_np(t, np.int64) for t in (row_id, inv, list_off, assignment))
    N, nlist = len(assignment), len(list_off) - 1
    assert row_id.shape == (N,) and inv.shape == (N,), (row_id.shape, inv.shape, N)
    assert np.array_equal(np.sort(row_id), np.arange(N)), "the lists do not partition 0 .. N - 1"
    assert np.array_equal(inv[row_id], np.arange(N)) and np.array_equal(row_id[inv], np.arange(N)), "inv is not the inverse of row_id"
    assert list_off[0] == 0 and list_off[-1] == N and (np.diff(list_off) >= 0).all(), ("offsets", list_off[:4], list_off[-1])
    assert np.array_equal(np.diff(list_off), np.bincount(assignment, minlength=nlist)), "list lengths differ from the assignment"
    for l in range(nlist):
        rows = row_id[list_off[l]:list_off[l + 1]]
        assert (assignment[rows] == l).all(), ("a row in a list it is not assigned to", l)
        assert (np.diff(rows) > 0).all(), ("rows do not ascend inside a list", l)


FAULTS = ("ties_by_position", "drop_last", "skip_unmapped", "fold_twice")


def model_ivf(scores, assignment, probes, k, skip=None, fault=None):
    """Scan + fold on the host.  The catalogue is stored list by list (a stable sort of the assignment); each probed list gives the k
    best of its rows by (score descending, original row ascending), the row at the position of the query's skipped original row left
    out; the fold keeps the k best of a query's lists.  fault: one of FAULTS --
      ties_by_position  equal scores ordered by the permuted position instead of the original row
      drop_last         the last row of every list is never scanned
      skip_unmapped     skip taken as a position without the inverse permutation
      fold_twice        a query's first probe folded twice"""
    assert fault is None or fault in FAULTS
    scores, assignment, probes = np.asarray(scores), _np(assignment, np.int64), _np(probes, np.int64)
    B, N = scores.shape
    row_id = np.argsort(assignment, kind="stable")
    inv = np.empty(N, np.int64)
    inv[row_id] = np.arange(N)
    list_off = np.concatenate([[0], np.cumsum(np.bincount(assignment, minlength=int(assignment.max()) + 1))])
    idx = np.full((B, k), -1, np.int64)
    sc = np.full((B, k), -np.inf, np.float32)
    for b in range(B):
        sk = -1
        if skip is not None and 0 <= int(skip[b]) < N:
            sk = int(skip[b]) if fault == "skip_unmapped" else int(inv[int(skip[b])])
        lists = []
        for l in probes[b][probes[b] >= 0]:
            lo, hi = int(list_off[l]), int(list_off[l + 1])
            if fault == "drop_last" and hi > lo:
                hi -= 1
            ent = [(-float(scores[b, row_id[p]]), p if fault == "ties_by_position" else int(row_id[p]), int(row_id[p]))
                   for p in range(lo, hi) if p != sk]
            lists.append(sorted(ent)[:k])
        if fault == "fold_twice" and lists:
            lists.append(lists[0])
        best = sorted(e for ent in lists for e in ent)[:k]
        for a, (ns, _, row) in enumerate(best):
            idx[b, a], sc[b, a] = row, -ns
    return idx, sc
