"""fp64 reference of the knowledge-graph pretraining kernels (csrc/kgpretrain.hip), in plain torch with autograd and no call into
the HIP library: one ia_kgpt_score step (PKGM / TransE, L1 / L2), coupled-L2 Adam and row normalisation.

`score_step` also returns, per element of every output, an error scale S for the bound |got - ref| <= tau * S.  S is the fp64
sum of the absolute values of everything the element is built from: the same forward and backward evaluated on |.| of every
operand (|hn|, |r|, |tn|, |P|, |upstream|), so an element that is small because of cancellation still gets the scale of the terms
that cancelled.  A table gradient's S is the sum of that over the element's occurrences, so a dropped or duplicated occurrence
shows up as an error of about S / (number of occurrences), while fp32 rounding stays at a few 1e-7 of S.

For L1 the subgradient is sign(x) with sign(0) = 0 (torch's abs).  On random data an x within fp32 rounding of zero may take
either sign in the kernel; with `sign_tol=True` such elements get the subgradient 0 in the reference and their largest possible
effect (|upstream| per element, carried through the same backward on |.|) is returned as U, to be added to the bound.  On the
exact binary grids of the edge tests every sign is exact and `sign_tol` stays off.
"""
import math

import torch
import torch.nn.functional as F

F64 = torch.float64
EPS32 = 2.0 ** -23
NORM_EPS = 1e-12          # F.normalize default


def f32(x):
    """x rounded to fp32, as a Python float (the kernels take margin / lr / ... as fp32)."""
    return float(torch.tensor(x, dtype=torch.float32))


def _gather(table, idx, n):
    """Rows table[idx] as a leaf; ids outside [0, n) read as zero rows and get no gradient (the kernels' contract)."""
    ok = (idx >= 0) & (idx < n)
    rows = table[idx.clamp(0, n - 1)] * ok[:, None].to(table.dtype)
    return rows.detach().requires_grad_(), ok


def _dist(x, norm, sgn=None):
    """torchkge's dissimilarity per row: |x|_1 or |x|_2^2.  With sgn, L1 takes that subgradient instead of sign(x)."""
    if norm == 2:
        return x.pow(2).sum(-1)
    if sgn is None:
        return x.abs().sum(-1)
    return x.detach().abs().sum(-1) + ((x - x.detach()) * sgn).sum(-1)


def _scatter(n, D, idx, ok, rows, dev):
    out = torch.zeros(n, D, dtype=F64, device=dev)
    return out.index_add_(0, idx[ok], rows[ok])


def score_step(ent, rel, proj, h, t, r, nh, nt, norm, *, margin=None, dpos=None, dneg=None, active=None, sign_tol=False):
    """One ia_kgpt_score step in fp64 on the device of `ent`.

    proj None = TransE.  Either margin (MarginLoss, reduction 'sum'; with `active` [B] bool the hinge decisions are taken from it
    instead of fp64) or an upstream (dpos, dneg) for sum(dpos * pos + dneg * neg).  Returns a dict: pos, neg, loss (None for an
    upstream), act (the hinge decisions used), grad_{ent,rel,proj}, S_{pos,neg,ent,rel,proj}, U_{ent,rel,proj}, count_{ent,rel}
    (occurrences per table row) and drop_{ent,rel} (per occurrence with a non-zero gradient: max over the row of |its
    contribution| / S, the relative error that losing it would leave)."""
    dev = ent.device
    E, R = ent.detach().to(F64), rel.detach().to(F64)
    P = None if proj is None else proj.detach().to(F64).requires_grad_()
    B, D = h.numel(), E.shape[1]
    n_ent, n_rel = E.shape[0], R.shape[0]
    heads, tails, rels = torch.cat([h, nh]), torch.cat([t, nt]), torch.cat([r, r])
    Hr, okh = _gather(E, heads, n_ent)
    Tr, okt = _gather(E, tails, n_ent)
    Rr, okr = _gather(R, rels, n_rel)
    hn, tn = F.normalize(Hr, p=2, dim=1), F.normalize(Tr, p=2, dim=1)
    u = hn + Rr - tn
    hp = hn @ P.T if P is not None else None
    w = hp - Rr if P is not None else None

    # magnitudes of the forward (the same expressions on |.|)
    a, ra, ta = hn.detach().abs(), Rr.detach().abs(), tn.detach().abs()
    ua = a + ra + ta
    hpa = a @ P.detach().abs().T if P is not None else None
    wa = hpa + ra if P is not None else None

    sgn_u = sgn_w = None
    frag_u = frag_w = None
    if norm == 1 and sign_tol:
        frag_u = u.detach().abs() <= 8 * EPS32 * ua
        sgn_u = torch.sign(u.detach()) * ~frag_u
        if P is not None:
            frag_w = w.detach().abs() <= EPS32 * (8 * ra + (8 + 4 * math.sqrt(D)) * hpa)
            sgn_w = torch.sign(w.detach()) * ~frag_w
    score = -_dist(u, norm, sgn_u)
    s_mag = (ua.pow(2) if norm == 2 else ua).sum(-1)
    if P is not None:
        score = score - _dist(w, norm, sgn_w)
        s_mag = s_mag + (wa.pow(2) if norm == 2 else wa).sum(-1)
    pos, neg = score[:B], score[B:]

    loss = None
    if margin is not None:
        margin = f32(margin)
        l = margin - pos + neg
        if active is None:
            act = (l >= 0).detach()
            loss = F.margin_ranking_loss(pos, neg, torch.ones_like(pos), margin=margin, reduction="sum")
        else:
            act = active.to(dev).bool()
            loss = torch.where(act, l, torch.zeros_like(l)).sum()
        total = loss
        g = torch.cat([-act.to(F64), act.to(F64)])
    else:
        act = None
        dp, dn = dpos.detach().to(dev, F64), dneg.detach().to(dev, F64)
        total = (dp * pos).sum() + (dn * neg).sum()
        g = torch.cat([dp, dn])
    total.backward()

    # backward on |.|: d hn, d tn, d r, d hp of each triple, then the normaliser backward, the tables and dP
    norms = Hr.detach().norm(dim=1), Tr.detach().norm(dim=1)
    ga = g.abs()[:, None]

    def propagate(du, dw):
        dhn = du if P is None else du + dw @ P.detach().abs()
        out = []
        for y, dy, n in ((a, dhn, norms[0]), (ta, du, norms[1])):
            big = (n >= NORM_EPS)[:, None]
            out.append(torch.where(big, (dy + y * (y * dy).sum(1, keepdim=True)) / n.clamp_min(NORM_EPS)[:, None], dy / NORM_EPS))
        s_ent = _scatter(n_ent, D, heads, okh, out[0], dev) + _scatter(n_ent, D, tails, okt, out[1], dev)
        s_rel = _scatter(n_rel, D, rels, okr, du if P is None else du + dw, dev)
        s_proj = None if P is None else dw.T @ a
        return s_ent, s_rel, s_proj

    dua = ga * (2 * ua if norm == 2 else torch.ones_like(ua))
    dwa = None if P is None else ga * (2 * wa if norm == 2 else torch.ones_like(wa))
    S_ent, S_rel, S_proj = propagate(dua, dwa)
    if frag_u is not None:
        U_ent, U_rel, U_proj = propagate(ga * frag_u, None if P is None else ga * frag_w)
    else:
        U_ent, U_rel = torch.zeros_like(S_ent), torch.zeros_like(S_rel)
        U_proj = None if P is None else torch.zeros_like(S_proj)

    grad_ent = _scatter(n_ent, D, heads, okh, Hr.grad, dev) + _scatter(n_ent, D, tails, okt, Tr.grad, dev)
    grad_rel = _scatter(n_rel, D, rels, okr, Rr.grad, dev)
    ones = torch.ones(2 * B, 1, dtype=F64, device=dev)
    count_ent = (_scatter(n_ent, 1, heads, okh, ones, dev) + _scatter(n_ent, 1, tails, okt, ones, dev))[:, 0]
    count_rel = _scatter(n_rel, 1, rels, okr, ones, dev)[:, 0]

    def drop(rows, idx, ok, S):
        c = rows.abs()[ok]
        s = S[idx[ok]]
        q = (c / torch.where(s > 0, s, torch.ones_like(s))).amax(1)
        return q[c.amax(1) > 0]

    drop_ent = torch.cat([drop(Hr.grad, heads, okh, S_ent), drop(Tr.grad, tails, okt, S_ent)])
    drop_rel = drop(Rr.grad, rels, okr, S_rel)
    return dict(pos=pos.detach(), neg=neg.detach(), loss=None if loss is None else loss.detach(), act=act,
                grad_ent=grad_ent, grad_rel=grad_rel, grad_proj=None if P is None else P.grad,
                S_pos=s_mag[:B], S_neg=s_mag[B:], S_ent=S_ent, S_rel=S_rel, S_proj=S_proj, U_ent=U_ent, U_rel=U_rel, U_proj=U_proj,
                count_ent=count_ent, count_rel=count_rel, drop_ent=drop_ent, drop_rel=drop_rel)


def scores(ent, rel, proj, h, t, r, nh, nt, norm):
    """(pos, neg) in fp64 without gradients (picking a margin away from the hinge)."""
    with torch.no_grad():
        E, R = ent.to(F64), rel.to(F64)
        heads, tails, rels = torch.cat([h, nh]), torch.cat([t, nt]), torch.cat([r, r])
        hn, tn = F.normalize(_gather(E, heads, E.shape[0])[0], p=2, dim=1), F.normalize(_gather(E, tails, E.shape[0])[0], p=2, dim=1)
        rv = _gather(R, rels, R.shape[0])[0]
        s = -_dist(hn + rv - tn, norm)
        if proj is not None:
            s = s - _dist(hn @ proj.to(F64).T - rv, norm)
        B = h.numel()
        return s[:B].detach(), s[B:].detach()


def adam_l2(p, m, v, grads, lrs, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=0.0, first_step=1):
    """torch.optim.Adam's single-tensor step with coupled L2 (grad + weight_decay * param), in fp64, one step per (grad, lr);
    the first of them is step `first_step` (counted from 1).  Returns (p, m, v, S_p, S_m, S_v): S_* the sum over the steps of the magnitudes of every term that
    enters the value (the error scale of an fp32 run)."""
    p, m, v = (x.to(F64).clone() for x in (p, m, v))
    Sp, Sm, Sv = p.abs(), m.abs(), v.abs()
    for step, (g, lr) in enumerate(zip(grads, lrs), first_step):
        ga = g.to(F64).abs() + weight_decay * p.abs()
        g = g.to(F64) + weight_decay * p
        m = m + (1 - beta1) * (g - m)                 # lerp(m, g, 1 - beta1)
        v = v * beta2 + (1 - beta2) * g * g
        step_size = lr / (1 - beta1 ** step)
        bc2_sqrt = math.sqrt(1 - beta2 ** step)
        Sm = beta1 * Sm + (1 - beta1) * ga + m.abs()
        Sv = beta2 * Sv + (1 - beta2) * ga * ga + v
        denom = v.sqrt() / bc2_sqrt + eps
        p = p - step_size * m / denom
        Sp = Sp + p.abs() + step_size * 2 * Sm / denom
    return p, m, v, Sp, Sm, Sv


def row_normalize(x):
    """x / max(|x|_2, 1e-12) per row in fp64 (F.normalize)."""
    return F.normalize(x.to(F64), p=2, dim=1)
