"""fp64 reference of ia_contrastive_fwd / ia_contrastive_bwd (include/itemalign.h) with the error bounds the GPU test holds the kernels to.

With s = exp(log_scale), from the same fp32 text / image [B, H] and log_scale the kernels get:
  sim = s text image^T; lse_row_i = log sum_j exp(sim_ij); lse_col_j = log sum_i exp(sim_ij);
  loss = 0.5 (mean_i (lse_row_i - sim_ii) + mean_j (lse_col_j - sim_jj))    [= 0.5 (CE(sim, arange) + CE(sim^T, arange))]
  G_ij = dloss (0.5 / B) (exp(sim_ij - lse_row_i) + exp(sim_ij - lse_col_j) - 2 [i == j])
  dtext = s G image; dimage = s G^T text; dlog_scale = sum_ij G_ij sim_ij.

Bounds.  u = 2^-24 (half an fp32 ulp); chain lengths are those csrc/contrastive.hip states in its header comment.
  * sim: a dot product of H terms through dot_chain(H) = ceil(H / 4) + 2 roundings, c u sum_k |t_ik i_jk|; s = expf(log_scale) is 1 ulp
    = 2 u relative (HIP's documented maximum for expf and logf), the product with s one more rounding: 3 u |sim|.
  * lse: log-sum-exp moves by at most the largest perturbation of its arguments, so the kernel's lse of its own sim is within max_j
    sim_bound_ij of the lse of the exact sim.  Its own arithmetic, with m the maximum, d_j = m - x_j, p_j the softmax: x_j - m one rounding
    (u d_j relative in e_j), expf 2 u, the sum of the positive e_j through wave_chain(B) = ceil(B / 64) + 6 roundings, logf 2 u |log S|,
    the addition u |lse|.  Through the logarithm the first three weigh in as sum_j p_j (u d_j + 2 u + c u), and sum_j p_j d_j = lse -
    sum_j p_j x_j is the entropy of p, at most ln B, as is log S: u (2 + c + 3 ln B) + u |lse|, whatever the perturbation of sim did to p.
  * loss: r_i = lse_row_i - sim_ii has the bounds of both and one rounding; the means are sums of B non-negative terms through
    wave_chain(B) roundings, two divisions side by side and an addition (2 more); the product with 0.5 is exact.
  * G: the argument a = sim_ij - lse_i is off by da = sim_bound_ij + lse_bound_i + u |a|, so p = exp(a) by the factor exp(+-da), and expf
    adds 2 u: |p' - p| <= p expm1(da + 2 u) -- not linearised, da reaches 1 where |sim| is 1e4.  c = dloss * (0.5f / B) is two
    roundings, (p + q) - 2 [i == j] two (of |p + q| and of the difference), the product one.
  * dtext / dimage: dot products of B terms, dot_chain(B) roundings of sum_j |G_ij x_jk|, the error of G carried through |x|, 3 u for s
    and the product with it.  dlog_scale: rows of B terms through wave_chain(B), the B row parts through wave_chain(B) again, one more
    rounding when it accumulates; the errors of G and sim carried through the products.
Second-order terms are covered by the factor SLACK; TINY is added wherever a result may fall below the fp32 normal range and be flushed.
"""
import math

import torch

F64 = torch.float64
U24 = 2.0 ** -24
TINY = 2.0 ** -125
SLACK = 1.0 + 2.0 ** -10


def dot_chain(n):
    """roundings on the longest path of an n-term dot product kept in four accumulators and combined as (a0 + a1) + (a2 + a3)"""
    return math.ceil(n / 4) + 2


def wave_chain(n):
    """n terms summed by one wave: ceil(n / 64) per lane, 4 butterfly steps + 2 across the 16-lane rows"""
    return math.ceil(n / 64) + 6


def forward(text, image, log_scale):
    """text, image [B, ld >= H is the caller's business: pass the [B, H] part] fp32, log_scale a float -> dict of fp64 tensors: sim,
    lse_row, lse_col, loss (0-d) and their bounds sim_bound [B, B], lse_row_bound, lse_col_bound [B], loss_bound (0-d)."""
    t, im = text.to(F64), image.to(F64)
    B, H = t.shape
    s = math.exp(float(log_scale))
    sim = s * (t @ im.T)
    sim_bound = SLACK * (s * dot_chain(H) * U24 * (t.abs() @ im.abs().T) + 3 * U24 * sim.abs()) + TINY
    own = U24 * (2 + wave_chain(B) + 3 * math.log(B)) + B * 2.0 ** -126
    lse_row = torch.logsumexp(sim, dim=1)
    lse_col = torch.logsumexp(sim, dim=0)
    lse_row_bound = SLACK * (sim_bound.max(dim=1).values + own + U24 * lse_row.abs())
    lse_col_bound = SLACK * (sim_bound.max(dim=0).values + own + U24 * lse_col.abs())
    diag, diag_bound = sim.diagonal(), sim_bound.diagonal()
    r, c = lse_row - diag, lse_col - diag
    term_err = (lse_row_bound + diag_bound + U24 * r.abs()).sum() + (lse_col_bound + diag_bound + U24 * c.abs()).sum()
    loss = 0.5 * (r.mean() + c.mean())
    loss_bound = SLACK * (0.5 / B) * (term_err + (wave_chain(B) + 2) * U24 * (r.abs().sum() + c.abs().sum())) + TINY
    return dict(sim=sim, lse_row=lse_row, lse_col=lse_col, loss=loss, sim_bound=sim_bound, lse_row_bound=lse_row_bound,
                lse_col_bound=lse_col_bound, loss_bound=loss_bound, scale=s)


def backward(text, image, log_scale, dloss=1.0, fwd=None, accumulated_onto=0.0):
    """-> dict of fp64 tensors: G [B, B], dtext, dimage [B, H], dlog_scale (0-d, accumulated_onto included) and the bounds G_bound,
    dtext_bound, dimage_bound, dlog_scale_bound."""
    f = forward(text, image, log_scale) if fwd is None else fwd
    t, im = text.to(F64), image.to(F64)
    B, H = t.shape
    s, sim, sb = f["scale"], f["sim"], f["sim_bound"]
    c = float(dloss) * 0.5 / B
    a_row, a_col = sim - f["lse_row"].view(-1, 1), sim - f["lse_col"].view(1, -1)
    p, q = torch.exp(a_row), torch.exp(a_col)
    eye = torch.eye(B, dtype=F64)
    inner = p + q - 2 * eye
    G = c * inner
    p_err = p * torch.expm1(sb + f["lse_row_bound"].view(-1, 1) + U24 * a_row.abs() + 2 * U24)
    q_err = q * torch.expm1(sb + f["lse_col_bound"].view(1, -1) + U24 * a_col.abs() + 2 * U24)
    G_bound = SLACK * (abs(c) * (p_err + q_err + U24 * (p + q)) + 4 * U24 * G.abs()) + TINY
    cb = dot_chain(B)
    dtext, dimage = s * (G @ im), s * (G.T @ t)
    dtext_bound = SLACK * (s * (G_bound @ im.abs() + cb * U24 * (G.abs() @ im.abs())) + 3 * U24 * dtext.abs()) + TINY
    dimage_bound = SLACK * (s * (G_bound.T @ t.abs() + cb * U24 * (G.abs().T @ t.abs())) + 3 * U24 * dimage.abs()) + TINY
    fresh = (G * sim).sum()
    dls = fresh + accumulated_onto
    carried = (G_bound * sim.abs() + G.abs() * sb + G_bound * sb).sum()
    dls_bound = SLACK * (carried + 2 * wave_chain(B) * U24 * (G * sim).abs().sum() + U24 * abs(float(dls))) + TINY
    return dict(G=G, dtext=dtext, dimage=dimage, dlog_scale=dls, G_bound=G_bound, dtext_bound=dtext_bound, dimage_bound=dimage_bound,
                dlog_scale_bound=dls_bound)


# ---- the inputs both test files use
SHAPES = [(1, 64), (2, 64), (3, 128), (17, 192), (64, 768), (65, 768), (257, 128)]
LOG_SCALES = [0.0, 1.0, -3.0, 4.6]
KINDS = ["random", "equal", "spike", "huge"]


def build(B, H, kind, seed):
    """fp32 text, image [B, H].  random: N(0, 1) / sqrt(H) rows scaled so that sim is O(1) before log_scale; equal: every row the same
    vector (sim constant, loss = ln B); spike: random, with sim[0][B - 1] (off the diagonal from B = 2 on) lifted by 80 above the O(1)
    rest at log_scale 0; huge: magnitudes that put sim at +-1e4 at log_scale 0."""
    g = torch.Generator().manual_seed(seed)
    t = torch.randn(B, H, generator=g)
    im = torch.randn(B, H, generator=g)
    if kind == "random":
        t, im = t / H ** 0.25, im / H ** 0.25
    elif kind == "equal":
        t, im = t[:1].repeat(B, 1) / H ** 0.25, im[:1].repeat(B, 1) / H ** 0.25
    elif kind == "spike":
        t, im = t / H ** 0.25, im / H ** 0.25
        # add to text row 0 the multiple of image row B - 1 that lifts sim[0][B - 1] by 80
        v = im[B - 1]
        t[0] = t[0] + v * (80.0 / float(v @ v))
    elif kind == "huge":
        a = (1e4 / H ** 0.5) ** 0.5          # a dot product of H terms of variance a^4 has the standard deviation 1e4
        t, im = t * a, im * a
    else:
        raise ValueError(kind)
    return t.to(torch.float32).contiguous(), im.to(torch.float32).contiguous()
