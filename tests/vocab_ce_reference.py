"""fp64 reference of ia_vocab_ce_fwd / ia_vocab_ce_bwd (include/itemalign.h) with the error bounds the GPU test holds the kernels to.

Semantics (those of the kernels, and of nn.CrossEntropyLoss(ignore_index=-1) wherever torch defines them):
  * a row with label < 0 is ignored: lse = loss_row = 0 (the kernel reads nothing of it), its dlogits row is zero, it is not counted;
  * a label >= V: lse as usual, loss_row = NaN (hence the mean), its dlogits row is zero, it counts as labelled;
  * mean = sum of loss_row over the labelled rows / their number, NaN when there is none;
  * dlogits[r, j] = (exp(x_rj - lse_r) - [j == label_r]) * dloss / n_live for j < V, zero in the pad columns.

Bounds.  u = 2^-24 (half an fp32 ulp).  The kernel's operations and their first-order errors, per row, with m = the row maximum (exact),
d_j = m - x_j >= 0, e_j = exp(-d_j), S = sum e_j >= 1:
  * x_j - m is one rounding, u d_j of absolute error in the argument, i.e. u d_j of relative error in e_j;
  * expf / logf are the device library's, 1 ulp = 2 u relative (HIP's documented maximum for both);
  * the sum of the positive e_j through a chain of c roundings: c u S (and 2^-126 per term that may be flushed as a subnormal);
  * lse = m + logf(S): err(S) / S through the logarithm, 2 u |log S| for logf, u |lse| for the addition;
  * loss_row = lse - x_label: one more rounding.
Second-order terms are some 2^-24 of these and are covered by the factor SLACK; TINY is added wherever a result may fall below the
fp32 (bf16) normal range and be flushed.
"""
import math

import torch

F64 = torch.float64
U24 = 2.0 ** -24
BF16_ULP = 2.0 ** -8
TINY = 2.0 ** -125
SLACK = 1.0 + 2.0 ** -10
THREADS, ROWS_PER_PART = 256, 1024      # csrc/vocab_ce.hip


def row_chain(V):
    """roundings on the longest path of one row's sum of exponentials: ceil(V / 1024) quads per thread, 2 inside a quad, 1 for the tail
    element, 6 for the wave reduction (4 butterfly steps + 2 across the 16-lane rows), 3 across the four waves"""
    return math.ceil((V // 4) / THREADS) + 2 + 1 + 6 + 3


def mean_chain(M):
    """the mean: 4 rows per thread, 6 + 3 for the workgroup of stage 1; ceil(parts / 64) per lane and 6 in stage 2; the division"""
    parts = math.ceil(M / ROWS_PER_PART)
    return 4 + 6 + 3 + math.ceil(parts / 64) + 6 + 1


def forward(logits, labels, V):
    """logits [M, ld] (any float dtype; columns >= V ignored), labels [M] int64 -> dict of fp64 tensors: lse, loss_row, mean (0-d), n_live
    (int) and the bounds lse_bound, loss_row_bound [M], mean_bound (0-d)."""
    x = logits[:, :V].to(F64)
    M = x.shape[0]
    live = labels >= 0
    oob = labels >= V
    m = x.max(dim=1, keepdim=True).values
    d = m - x
    e = torch.exp(-d)
    S = e.sum(dim=1)
    lse = (m.squeeze(1) + torch.log(S))
    c = row_chain(V)
    err_S = (e * (2 * U24 + U24 * d)).sum(dim=1) + V * 2.0 ** -126 + c * U24 * S
    lse_bound = SLACK * (err_S / S + 2 * U24 * torch.log(S).abs() + U24 * lse.abs())
    safe = labels.clamp(0, V - 1)
    picked = x.gather(1, safe.view(-1, 1)).squeeze(1)
    loss_row = lse - picked
    loss_row_bound = SLACK * (lse_bound + U24 * loss_row.abs()) + TINY
    zero = torch.zeros((), dtype=F64)
    lse = torch.where(live, lse, zero)
    lse_bound = torch.where(live, lse_bound, zero)
    loss_row = torch.where(live, loss_row, zero)
    loss_row = torch.where(oob, torch.full((), float("nan"), dtype=F64), loss_row)
    loss_row_bound = torch.where(live, loss_row_bound, zero)
    n = int(live.sum())
    if n == 0:
        mean = torch.full((), float("nan"), dtype=F64)
        mean_bound = zero.clone()
    else:
        mean = loss_row[live].sum() / n
        mean_bound = SLACK * (loss_row_bound[live].sum() + mean_chain(M) * U24 * loss_row[live].abs().sum()) / n
    return dict(lse=lse, loss_row=loss_row, mean=mean, n_live=n, lse_bound=lse_bound, loss_row_bound=loss_row_bound, mean_bound=mean_bound)


def backward(logits, labels, V, ldg, dloss=1.0, fwd=None):
    """-> (dlogits fp64 [M, ldg], fp32_bound [M, ldg]): the gradient and the bound of the kernel's fp32 arithmetic in front of the bf16
    rounding.  p = expf(x - lse'), lse' the kernel's own lse (within lse_bound of the true one): relative error 2 u (expf) + u |x - lse|
    (the subtraction) + lse_bound; p - onehot and the product with scale = dloss / n (itself one rounding) are three more roundings of
    the result.  Zero -- exactly -- in ignored rows, rows whose label is outside the vocabulary, and the pad columns."""
    fwd = forward(logits, labels, V) if fwd is None else fwd
    x = logits[:, :V].to(F64)
    M = x.shape[0]
    g = torch.zeros((M, ldg), dtype=F64)
    b = torch.zeros((M, ldg), dtype=F64)
    rows = (labels >= 0) & (labels < V)
    n = fwd["n_live"]
    if n == 0 or not rows.any():
        return g, b
    scale = float(dloss) / n
    lse = fwd["lse"].view(-1, 1)
    p = torch.exp(x - lse)
    onehot = torch.zeros_like(x)
    onehot[rows, labels[rows]] = 1.0
    val = (p - onehot) * scale
    p_err = p * (2 * U24 + U24 * (x - lse).abs() + fwd["lse_bound"].view(-1, 1))
    bound = SLACK * abs(scale) * (p_err + 3 * U24 * (p - onehot).abs()) + TINY
    g[rows, :V] = val[rows]
    b[rows, :V] = bound[rows]
    return g, b
