"""Plain-torch fp64 reference of link-prediction ranking (torchkge LinkPredictionEvaluator over TranslationModel's
inference_scoring_function, filter_scores and get_rank), with an error scale per candidate and the rank bracket a correct fp32 kernel
must land in.

Query vector, in fp64 from the fp32 tables: tail side q = ent[h] + rel[r] (true entity t), head side q = ent[t] - rel[r] (true h).
Score s_c = -d(q, ent[c]); d = |q - c|_2^2 (norm 2) or |q - c|_1 (norm 1).  Error scale S_c = (|q|_2 + |c|_2)^2 (norm 2) or
|q|_1 + |c|_1 (norm 1): fp32 rounding of the query, the differences and the sum moves d by a small multiple of S_c.

Bracket of a query with true entity e and filtered set F (F empty for the raw rank), tau = 1e-5:
    lo = 1 + #{c != e, c not in F : s_c > s_e + tau (S_c + S_e)}
    hi = 1 + #{c != e, c not in F : s_c >= s_e - tau (S_c + S_e)}
"""
import torch

TAU = 1e-5
TAIL, HEAD = 0, 1


def query_vectors(ent, rel, h, t, r, side):
    ent, rel = ent.double(), rel.double()
    return ent[h] + rel[r] if side == TAIL else ent[t] - rel[r]


def scores_fp64(ent, rel, h, t, r, norm, side, chunk=256):
    """(s [B, n_ent], S [B, n_ent]) in fp64 on ent's device, computed in query chunks (direct differences, no GEMM expansion)."""
    q = query_vectors(ent, rel, h, t, r, side)
    c = ent.double()
    p = 2.0 if norm == 2 else 1.0
    cn = c.norm(p=p, dim=1)
    s, S = [], []
    for i in range(0, q.shape[0], chunk):
        qq = q[i:i + chunk]
        d = torch.cdist(qq, c, p=p, compute_mode="donot_use_mm_for_euclid_dist")
        qn = qq.norm(p=p, dim=1)
        if norm == 2:
            s.append(-(d * d))
            S.append((qn[:, None] + cn[None, :]) ** 2)
        else:
            s.append(-d)
            S.append(qn[:, None] + cn[None, :])
    return torch.cat(s), torch.cat(S)


def true_ids(h, t, side):
    return t if side == TAIL else h


def bracket(s, S, true, filt_mask=None, tau=TAU):
    """(lo, hi) int64 [B]; filt_mask [B, n_ent] bool marks the filtered candidates (the true id may be marked: it is skipped anyway)."""
    B = s.shape[0]
    ar = torch.arange(B, device=s.device)
    st, St = s[ar, true][:, None], S[ar, true][:, None]
    keep = torch.ones_like(s, dtype=torch.bool)
    keep[ar, true] = False
    if filt_mask is not None:
        keep &= ~filt_mask
    tol = tau * (S + St)
    lo = 1 + ((s > st + tol) & keep).sum(1)
    hi = 1 + ((s >= st - tol) & keep).sum(1)
    return lo, hi


def near_tie(s, S, true, tau=1e-4):
    """bool [B]: some candidate other than the true one scores within tau (S_c + S_e) of the true score."""
    B = s.shape[0]
    ar = torch.arange(B, device=s.device)
    st, St = s[ar, true][:, None], S[ar, true][:, None]
    close = (s - st).abs() <= tau * (S + St)
    close[ar, true] = False
    return close.any(1)


def filter_mask(groups, q_grp, n_ent, device=None):
    """[B, n_ent] bool of the members of each query's group (FilterGroups, group indices; -1 = none)."""
    m = torch.zeros(len(q_grp), n_ent, dtype=torch.bool, device=device)
    for i, g in enumerate(q_grp):
        if g >= 0:
            ids = torch.as_tensor(groups.members(int(g)), dtype=torch.int64, device=device)
            m[i, ids] = True
    return m


def exact_rank(s, true, filt_mask=None):
    """torchkge's get_rank on fp64 scores: #{c : s_c >= s_e} with the filtered candidates (not the true one) at -inf."""
    B = s.shape[0]
    ar = torch.arange(B, device=s.device)
    x = s.clone()
    if filt_mask is not None:
        m = filt_mask.clone()
        m[ar, true] = False
        x[m] = -float("inf")
    return (x >= x[ar, true][:, None]).sum(1)
