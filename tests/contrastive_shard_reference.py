"""fp64 reference of ia_contrastive_shard_fwd / ia_contrastive_shard_bwd (include/itemalign.h) with the error bounds the GPU test holds
the kernels to.  One rank of `world` holds rows o .. o + B - 1 (o = row_offset) of a global batch of G items whose embeddings text_g,
image_g [G, H] every rank has; den = G / world, s = exp(log_scale), d = o + i:
  sim_t = s text_g[o:o+B] image_g^T [B, G] (rows o + i of the global sim), sim_i = s image_g[o:o+B] text_g^T (its columns o + i);
  lse_row_l, lse_col_l: their row log-sum-exps, the global lse_row / lse_col at o + i;
  loss = 0.5 (sum_i (lse_row_l[i] - sim_t[i][d]) / den + sum_i (lse_col_l[i] - sim_i[i][d]) / den)
  c = dloss 0.5 / den, with lse_row_g, lse_col_g [G] of the global matrix:
  Gt[i][j] = c (exp(sim_t[i][j] - lse_row_g[d]) + exp(sim_t[i][j] - lse_col_g[j]) - 2 [j == d]),
  Gi[i][j] = c (exp(sim_i[i][j] - lse_col_g[d]) + exp(sim_i[i][j] - lse_row_g[j]) - 2 [j == d]),
  dtext_l = s Gt image_g, dimage_l = s Gi text_g, dlog_scale = sum_ij Gt[i][j] sim_t[i][j].
The mean of the ranks' losses is the global loss; the ranks' dtext_l / dimage_l stacked and divided by world, and the sum of their
dlog_scale divided by world, are the global gradients (tests/test_contrastive_shard_reference_host.py holds this file to that).

Bounds: those of tests/contrastive_reference.py, whose derivation carries over term by term, with the chain lengths
csrc/contrastive.hip states for the shard entries.  Every sum that runs over the gathered rows has n = G: the sums of exponentials
(wave_chain(G), entropy at most ln G), a row's part of dlog_scale (wave_chain(G)) and the dot products of dtext_l / dimage_l
(dot_chain(G)).  The two sums of the loss and the sum of the row parts of dlog_scale run over the rank's own rows: wave_chain(B).
den = (float)G / (float)world is one rounding more than the square kernels' exact (float)B: one more on each of the loss's two
divisions, one more in c (3 roundings instead of 2; with the difference and the product, 5 u |G| instead of 4 u |G|).
"""
import math

import torch

from contrastive_reference import F64, SLACK, TINY, U24, dot_chain, wave_chain
import contrastive_reference as R


def forward(text_g, image_g, log_scale, row_offset, B, world):
    """text_g, image_g [G, H] fp32 -> dict of fp64 tensors: sim_t, sim_i [B, G], lse_row_l, lse_col_l [B], loss (0-d) and the bounds
    sim_t_bound, sim_i_bound, lse_row_l_bound, lse_col_l_bound, loss_bound."""
    tg, ig = text_g.to(F64), image_g.to(F64)
    G, H = tg.shape
    o = row_offset
    tl, il = tg[o:o + B], ig[o:o + B]
    s = math.exp(float(log_scale))
    den = G / world
    out = dict(scale=s, den=den)
    own = U24 * (2 + wave_chain(G) + 3 * math.log(G)) + G * 2.0 ** -126
    d = torch.arange(B) + o
    rows = torch.arange(B)
    term_err, term_abs = 0.0, 0.0
    for name, lse_name, a, b in (("sim_t", "lse_row_l", tl, ig), ("sim_i", "lse_col_l", il, tg)):
        sim = s * (a @ b.T)
        bound = SLACK * (s * dot_chain(H) * U24 * (a.abs() @ b.abs().T) + 3 * U24 * sim.abs()) + TINY
        lse = torch.logsumexp(sim, dim=1)
        lse_bound = SLACK * (bound.max(dim=1).values + own + U24 * lse.abs())
        r = lse - sim[rows, d]
        term_err = term_err + (lse_bound + bound[rows, d] + U24 * r.abs()).sum()
        term_abs = term_abs + r.abs().sum()
        out[name], out[name + "_bound"], out[lse_name], out[lse_name + "_bound"], out[name + "_term"] = sim, bound, lse, lse_bound, r
    out["loss"] = 0.5 * (out["sim_t_term"].sum() / den + out["sim_i_term"].sum() / den)
    out["loss_bound"] = SLACK * (0.5 / den) * (term_err + (wave_chain(B) + 3) * U24 * term_abs) + TINY
    return out


def backward(text_g, image_g, log_scale, row_offset, B, world, dloss=1.0, fwd=None, glob=None, accumulated_onto=0.0):
    """-> dict of fp64 tensors: Gt, Gi [B, G], dtext_l, dimage_l [B, H], dlog_scale (0-d, accumulated_onto included) and the bounds
    Gt_bound, Gi_bound, dtext_l_bound, dimage_l_bound, dlog_scale_bound.  glob: contrastive_reference.forward of the gathered batch,
    whose lse_row / lse_col (and their bounds) are the lse_row_g / lse_col_g the kernel is given."""
    f = forward(text_g, image_g, log_scale, row_offset, B, world) if fwd is None else fwd
    g = R.forward(text_g, image_g, log_scale) if glob is None else glob
    tg, ig = text_g.to(F64), image_g.to(F64)
    G, H = tg.shape
    s, den, o = f["scale"], f["den"], row_offset
    c = float(dloss) * 0.5 / den
    onehot = torch.zeros(B, G, dtype=F64)
    onehot[torch.arange(B), torch.arange(B) + o] = 1.0
    out = {}
    cb = dot_chain(G)
    for name, sim_name, own, other, src in (("Gt", "sim_t", "lse_row", "lse_col", ig), ("Gi", "sim_i", "lse_col", "lse_row", tg)):
        sim, sb = f[sim_name], f[sim_name + "_bound"]
        a_own, a_other = sim - g[own][o:o + B].view(-1, 1), sim - g[other].view(1, -1)
        p, q = torch.exp(a_own), torch.exp(a_other)
        M = c * (p + q - 2 * onehot)
        p_err = p * torch.expm1(sb + g[own + "_bound"][o:o + B].view(-1, 1) + U24 * a_own.abs() + 2 * U24)
        q_err = q * torch.expm1(sb + g[other + "_bound"].view(1, -1) + U24 * a_other.abs() + 2 * U24)
        M_bound = SLACK * (abs(c) * (p_err + q_err + U24 * (p + q)) + 5 * U24 * M.abs()) + TINY
        dx = s * (M @ src)
        dx_bound = SLACK * (s * (M_bound @ src.abs() + cb * U24 * (M.abs() @ src.abs())) + 3 * U24 * dx.abs()) + TINY
        dname = "dtext_l" if name == "Gt" else "dimage_l"
        out[name], out[name + "_bound"], out[dname], out[dname + "_bound"] = M, M_bound, dx, dx_bound
    Gt, Gb, sim, sb = out["Gt"], out["Gt_bound"], f["sim_t"], f["sim_t_bound"]
    dls = (Gt * sim).sum() + accumulated_onto
    carried = (Gb * sim.abs() + Gt.abs() * sb + Gb * sb).sum()
    out["dlog_scale"] = dls
    out["dlog_scale_bound"] = SLACK * (carried + (wave_chain(G) + wave_chain(B)) * U24 * (Gt * sim).abs().sum() + U24 * abs(float(dls))) + TINY
    return out


# ---- the inputs both test files use: (B, G, row_offset, H); the operand kinds and scales are contrastive_reference's
SHAPES = [(1, 1, 0, 64), (1, 2, 1, 64), (3, 7, 4, 128), (17, 65, 0, 192), (17, 65, 48, 192), (16, 257, 100, 128), (1, 257, 256, 128),
          (64, 128, 64, 768)]


def world_of(B, G):
    """a world size that goes with a shard of B rows out of G: the number of such shards, rounded"""
    return max(1, round(G / B))
