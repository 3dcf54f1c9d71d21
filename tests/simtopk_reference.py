"""References of same-item retrieval (ia_sim_rows_bf16, ia_sim_topk; csrc/simtopk.hip).  Host only: numpy and torch fp64.

* rows_fp64:   what ia_sim_rows_bf16 prepares, before the bf16 rounding: x, or x / max(|x|_2, 1e-12) row by row.
* scores_fp64: q c^T of the bf16 rows taken as exact numbers.
* bar:         (pitch + 2) * 2^-23 * (|q| |c|^T), the accumulator rule of tests/gemm_reference.py: the worst case of a length-pitch sum
               of fp32 adds in any order, doubled because the MFMA's internal adds are not individually rounded.
* select:      the k best ids per query in the total order (score descending, id ascending) by np.lexsort, one id set aside per query.
* check_topk:  what a kernel result must satisfy against the fp64 scores when its own scores carry rounding errors.
"""
import numpy as np
import torch

U = 2.0 ** -23


def rows_fp64(x, normalize):
    x = torch.as_tensor(x).to(torch.float64)
    if not normalize:
        return x
    return x / x.norm(dim=1, keepdim=True).clamp_min(1e-12)


def _f64(x):
    return np.asarray(torch.as_tensor(x).detach().cpu().to(torch.float64).numpy())


def scores_fp64(q, c):
    """fp64 numpy [B, n] from the (bf16) rows"""
    return _f64(q) @ _f64(c).T


def bar(q, c, pitch=None):
    q, c = _f64(q), _f64(c)
    pitch = q.shape[1] if pitch is None else pitch
    return (pitch + 2) * U * (np.abs(q) @ np.abs(c).T)


def select(scores, k, skip=None):
    """(idx int64 [B, k], score fp32 [B, k]) numpy, from a [B, n] score matrix; skip [B]: the id query b never gets (-1: none);
    unused slots -1 / -inf"""
    scores = np.asarray(scores)
    B, n = scores.shape
    idx = np.full((B, k), -1, np.int64)
    sc = np.full((B, k), -np.inf, np.float32)
    for i in range(B):
        ids = np.arange(n)
        if skip is not None and 0 <= int(skip[i]) < n:
            ids = ids[ids != int(skip[i])]
        s = scores[i, ids]
        order = np.lexsort((ids, -s))[:k]
        idx[i, :len(order)] = ids[order]
        sc[i, :len(order)] = s[order]
    return idx, sc


def check_topk(idx, score, s64, bars, k, skip=None):
    """Raises AssertionError unless (idx, score) is a valid answer for the fp64 scores s64 [B, n] with per-pair error bounds bars [B, n]:
      (i)   every returned score is within the bar of the fp64 score of its id;
      (ii)  each list is sorted by the kernel's own (score descending, id ascending), holds no id twice and not the skipped id;
      (iii) every candidate left out has an fp64 score <= the fp64 score of the k-th returned + the bars of the two;
      (iv)  unused slots (-1 / -inf, trailing) appear exactly when fewer than k candidates exist."""
    idx, score = np.asarray(torch.as_tensor(idx).cpu().numpy()), np.asarray(torch.as_tensor(score).cpu().numpy())
    s64, bars = np.asarray(s64), np.asarray(bars)
    B, n = s64.shape
    assert idx.shape == (B, k) and score.shape == (B, k), (idx.shape, score.shape, (B, k))
    for b in range(B):
        sk = int(skip[b]) if skip is not None and 0 <= int(skip[b]) < n else -1
        avail = n - (sk >= 0)
        used = min(k, avail)
        ids, sc = idx[b, :used], score[b, :used]
        assert (idx[b, used:] == -1).all() and np.isneginf(score[b, used:]).all(), ("(iv) unused slots", b, idx[b], score[b])
        assert ((ids >= 0) & (ids < n)).all() and np.isfinite(sc).all(), ("(iv) a used slot is empty or out of range", b, ids, sc)
        assert len(set(ids.tolist())) == used, ("(ii) an id twice", b, ids)
        assert sk not in ids.tolist(), ("(ii) the skipped id is returned", b, sk, ids)
        err = np.abs(sc.astype(np.float64) - s64[b, ids])
        assert (err <= bars[b, ids]).all(), ("(i) a score off its fp64 value", b, ids, sc, s64[b, ids], bars[b, ids])
        for a in range(used - 1):
            assert sc[a] > sc[a + 1] or (sc[a] == sc[a + 1] and ids[a] < ids[a + 1]), ("(ii) order", b, a, sc[a:a + 2], ids[a:a + 2])
        if used == k and avail > k:
            out = np.ones(n, bool)
            out[ids] = False
            if sk >= 0:
                out[sk] = False
            last = ids[-1]
            bad = out & (s64[b] > s64[b, last] + bars[b] + bars[b, last])
            assert not bad.any(), ("(iii) a better candidate is left out", b, np.nonzero(bad)[0][:5], s64[b, bad][:5], s64[b, last])


# ------------------------------------------------------------------------------------------------ a CPU model of the kernel
def model_topk(q, c, k, skip=None, seed=0, tile=128, ties_high=False, drop_tail=False, return_skipped=False):
    """The scan restated on the host: bf16 rows, fp32 accumulation in a permuted k order, candidate tiles of `tile` in shuffled arrival
    order, a running list of the k smallest keys (score descending, id ascending).  The three switches inject the faults check_topk
    has to catch."""
    rng = np.random.default_rng(seed)
    q32, c32 = (np.asarray(torch.as_tensor(x).detach().cpu().to(torch.float32).numpy()) for x in (q, c))
    B, n = q32.shape[0], c32.shape[0]
    perm = rng.permutation(q32.shape[1])
    acc = np.zeros((B, n), np.float32)
    for kk in perm:
        acc = (acc + q32[:, kk:kk + 1] * c32[None, :, kk]).astype(np.float32)
    tiles = [(lo, min(n, lo + tile)) for lo in range(0, n, tile)]
    if drop_tail and n % tile:
        tiles[-1] = (tiles[-1][0], tiles[-1][1] - 1)
    idx = np.full((B, k), -1, np.int64)
    sc = np.full((B, k), -np.inf, np.float32)
    for b in range(B):
        best = []                                             # (-score, +-id) tuples
        for t in rng.permutation(len(tiles)):
            lo, hi = tiles[t]
            for cid in range(lo, hi):
                if not return_skipped and skip is not None and cid == int(skip[b]):
                    continue
                best.append((-float(acc[b, cid]), -cid if ties_high else cid))
            best = sorted(best)[:k]
        for a, (ns, cid) in enumerate(best):
            idx[b, a], sc[b, a] = abs(cid), -ns
    return idx, sc
