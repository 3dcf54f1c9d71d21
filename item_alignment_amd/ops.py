"""Raw (non-autograd) Python entry points over the C ABI: argument checking, output allocation and the
`data_ptr()` plumbing.  Every function launches HIP kernels from libitemalign_hip.so on torch's current
stream; tensors must be CUDA(HIP)-resident and contiguous.  No function here computes with torch ops.
"""
import torch

from . import _lib
from ._lib import check, ptr, stream_ptr

EPI_NONE, EPI_BIAS, EPI_BIAS_GELU, EPI_ADD, EPI_DGELU, EPI_BIAS_ADD, EPI_DGELU_COLSUM = 0, 1, 2, 3, 4, 5, 6
ACT_NONE, ACT_TANH = 0, 1
BF16, F32 = torch.bfloat16, torch.float32


def _need(t, dtype, name):
    if t is None:
        return
    if not t.is_cuda:
        raise _lib.ItemAlignError(f"{name} must live on the GPU (the HIP path has no CPU fallback)")
    if t.dtype != dtype:
        raise TypeError(f"{name}: expected {dtype}, got {t.dtype}")
    if not t.is_contiguous():
        raise ValueError(f"{name} must be contiguous")


def gemm(a, b, *, a_kstrided=False, b_kstrided=False, epilogue=EPI_NONE, bias=None, aux=None, out=None, out_f32=False,
         accumulate=False, pre_out=None, colsum_out=None):
    """C = A*B (+epilogue).  a: [M,K] (or [K,M] if a_kstrided); b: [N,K] (or [K,N] if b_kstrided).
    EPI_DGELU_COLSUM also adds the column sums of C into colsum_out (fp32 [N])."""
    lib = _lib.load()
    _need(a, BF16, "a"); _need(b, BF16, "b"); _need(bias, F32, "bias"); _need(aux, BF16, "aux")
    if a_kstrided:
        K, M = a.shape
    else:
        M, K = a.shape
    if b_kstrided:
        Kb, N = b.shape
    else:
        N, Kb = b.shape
    if K != Kb:
        raise ValueError(f"gemm: inner dims differ ({K} vs {Kb})")
    if out is None:
        out = torch.empty((M, N), device=a.device, dtype=F32 if out_f32 else BF16)
    _need(out, F32 if out_f32 else BF16, "out")
    if epilogue == EPI_BIAS_GELU and pre_out is None:
        pre_out = torch.empty((M, N), device=a.device, dtype=BF16)
    ws_bytes = lib.ia_gemm_workspace_bytes(M, N, K, int(out_f32))
    if epilogue == EPI_DGELU_COLSUM:
        _need(colsum_out, F32, "colsum_out")
        if colsum_out is None:
            raise ValueError("gemm: EPI_DGELU_COLSUM needs colsum_out")
        pre_out = colsum_out
        ws_bytes = max(ws_bytes, lib.ia_gemm_colsum_workspace_bytes(M, N))
    ws = torch.empty(ws_bytes, device=a.device, dtype=torch.uint8) if ws_bytes else None
    check(lib.ia_gemm_bf16(a.data_ptr(), int(a_kstrided), a.shape[1], b.data_ptr(), int(b_kstrided), b.shape[1], out.data_ptr(),
                           int(out_f32), N, M, N, K, epilogue, ptr(bias), ptr(aux), N if aux is not None else 0, ptr(pre_out),
                           int(accumulate), ptr(ws), ws_bytes, stream_ptr()), "ia_gemm_bf16")
    if epilogue == EPI_BIAS_GELU:
        return out, pre_out
    return out


def _row_list(name, row_live):
    """One list or mask of the rows' live bytes (uint8 [M] on the GPU) -> int32 words: ia_<name>_bytes sizes it, ia_<name> builds it."""
    lib = _lib.load()
    _need(row_live, torch.uint8, "row_live")
    M = row_live.numel()
    out = torch.empty(getattr(lib, f"ia_{name}_bytes")(M) // 4, device=row_live.device, dtype=torch.int32)
    check(getattr(lib, f"ia_{name}")(row_live.data_ptr(), M, out.data_ptr(), stream_ptr()), f"ia_{name}")
    return out


def kblock_mask(row_live):
    """bit (b & 31) of word b >> 5 = any(row_live[32b : 32b + 32]) (uint8 [M] on the GPU) -> int32 words"""
    return _row_list("kblock_mask", row_live)


def gemm_wgrad_blocks(dy, x, mask=None, *, out=None, accumulate=False):
    """dW[N_out, N_in] (+)= dy[M, N_out]^T x[M, N_in] in fp32 over the 32-row blocks whose bit is set in `mask` (kblock_mask's int32
    words: a clear bit promises that the block's rows of dy are all zeros; ia_gemm_wgrad_blocks).  mask=None is the dense gemm."""
    lib = _lib.load()
    _need(dy, BF16, "dy"); _need(x, BF16, "x"); _need(mask, torch.int32, "mask")
    (M, n_out), (Mx, n_in) = dy.shape, x.shape
    if M != Mx or (mask is not None and mask.numel() * 4 != lib.ia_kblock_mask_bytes(M)):
        raise ValueError("gemm_wgrad_blocks: dy and x must have the same number of rows and mask ia_kblock_mask_bytes(M) bytes")
    if out is None:
        out = torch.empty((n_out, n_in), device=dy.device, dtype=F32)
    _need(out, F32, "out")
    ws_bytes = lib.ia_gemm_workspace_bytes(n_out, n_in, M, 1)
    ws = torch.empty(max(ws_bytes, 16), device=dy.device, dtype=torch.uint8)
    check(lib.ia_gemm_wgrad_blocks(dy.data_ptr(), n_out, x.data_ptr(), n_in, out.data_ptr(), n_in, n_out, n_in, M, ptr(mask),
                                   int(accumulate), ws.data_ptr(), ws_bytes, stream_ptr()), "ia_gemm_wgrad_blocks")
    return out


def kstep_mask(row_live):
    """bit (s & 31) of word s >> 5 = any(row_live[16s : 16s + 16]) (uint8 [M] on the GPU) -> int32 words"""
    return _row_list("kstep_mask", row_live)


def gemm_wgrad_steps(dy, x, mask=None, *, out=None, accumulate=False):
    """gemm_wgrad_blocks over the 16-row steps whose bit is set in `mask` (kstep_mask's int32 words; ia_gemm_wgrad_steps), four to a
    k-tile.  A shape whose k-slabs are too long for that walk (ia_gemm_wgrad_walk != 2) takes the block walk.  mask=None is the dense gemm."""
    lib = _lib.load()
    _need(dy, BF16, "dy"); _need(x, BF16, "x"); _need(mask, torch.int32, "mask")
    (M, n_out), (Mx, n_in) = dy.shape, x.shape
    if M != Mx or (mask is not None and mask.numel() * 4 != lib.ia_kstep_mask_bytes(M)):
        raise ValueError("gemm_wgrad_steps: dy and x must have the same number of rows and mask ia_kstep_mask_bytes(M) bytes")
    if out is None:
        out = torch.empty((n_out, n_in), device=dy.device, dtype=F32)
    _need(out, F32, "out")
    ws_bytes = lib.ia_gemm_wgrad_rows_workspace_bytes(n_out, n_in, M)      # (room for the block mask of a shape that walks blocks)
    ws = torch.empty(max(ws_bytes, 16), device=dy.device, dtype=torch.uint8)
    check(lib.ia_gemm_wgrad_steps(dy.data_ptr(), n_out, x.data_ptr(), n_in, out.data_ptr(), n_in, n_out, n_in, M, ptr(mask),
                                  int(accumulate), ws.data_ptr(), ws_bytes, stream_ptr()), "ia_gemm_wgrad_steps")
    return out


def gemm_wgrad_rows(dy, x, row_live=None, *, out=None, accumulate=False):
    """dW[N_out, N_in] (+)= dy[M, N_out]^T x[M, N_in] in fp32; row_live (uint8 [M]) == 0 promises that row of dy is all zeros, and
    32-row blocks without a live row are skipped (ia_gemm_wgrad_rows).  row_live=None is gemm(..., a_kstrided, b_kstrided, out_f32)."""
    lib = _lib.load()
    _need(dy, BF16, "dy"); _need(x, BF16, "x"); _need(row_live, torch.uint8, "row_live")
    (M, n_out), (Mx, n_in) = dy.shape, x.shape
    if M != Mx or (row_live is not None and row_live.numel() != M):
        raise ValueError("gemm_wgrad_rows: dy, x and row_live must have the same number of rows")
    if out is None:
        out = torch.empty((n_out, n_in), device=dy.device, dtype=F32)
    _need(out, F32, "out")
    ws_bytes = lib.ia_gemm_wgrad_rows_workspace_bytes(n_out, n_in, M)
    ws = torch.empty(ws_bytes, device=dy.device, dtype=torch.uint8)
    check(lib.ia_gemm_wgrad_rows(dy.data_ptr(), n_out, x.data_ptr(), n_in, out.data_ptr(), n_in, n_out, n_in, M, ptr(row_live),
                                 int(accumulate), ws.data_ptr(), ws_bytes, stream_ptr()), "ia_gemm_wgrad_rows")
    return out


def row_blocks(row_live):
    """The 32-row block list of ia_row_blocks (uint8 [M] on the GPU -> int32 words): [0] live count, [1] dead count, [2] blocks,
    the ascending live blocks from word 8, the ascending dead blocks from word 8 + blocks rounded up to 8."""
    return _row_list("row_blocks", row_live)


def row_slabs(row_live):
    """The 8-row slab list of ia_row_slabs (uint8 [M] on the GPU -> int32 words): [0] live count, [1] dead count, [2] slabs; from word 8
    the live slabs, 32 to a tile in the order [wave][piece] (-1 behind the last); the ascending dead slabs from word 8 + slabs rounded
    up to 32."""
    return _row_list("row_slabs", row_live)


def _gemm_dgrad_filtered(unit, dy, w, row_live, w_kstrided, epilogue, aux, out, colsum_out=None):
    """gemm_dgrad_rows (unit "rows": ia_gemm_dgrad_rows, the one with column sums) and gemm_dgrad_slabs ("slabs": ia_gemm_dgrad_slabs)"""
    lib = _lib.load()
    _need(dy, BF16, "dy"); _need(w, BF16, "w"); _need(aux, BF16, "aux"); _need(row_live, torch.uint8, "row_live")
    _need(colsum_out, F32, "colsum_out")
    M, K = dy.shape
    Kw, N = w.shape if w_kstrided else w.shape[::-1]
    if K != Kw or (row_live is not None and row_live.numel() != M):
        raise ValueError(f"gemm_dgrad_{unit}: dy, w and row_live do not fit together")
    slabs = unit == "slabs"
    if epilogue == EPI_DGELU_COLSUM and colsum_out is None and not slabs:
        raise ValueError("gemm_dgrad_rows: EPI_DGELU_COLSUM needs colsum_out")
    if out is None:
        out = torch.empty((M, N), device=dy.device, dtype=BF16)
    _need(out, BF16, "out")
    ws_bytes = lib.ia_gemm_slabs_workspace_bytes(M) if slabs else lib.ia_gemm_dgrad_rows_workspace_bytes(M, N, K)
    ws = torch.empty(ws_bytes, device=dy.device, dtype=torch.uint8)
    c2 = () if slabs else (ptr(colsum_out),)
    check(getattr(lib, f"ia_gemm_dgrad_{unit}")(dy.data_ptr(), K, w.data_ptr(), int(w_kstrided), w.shape[1], out.data_ptr(), N, M, N, K, epilogue,
                                                ptr(aux), N if aux is not None else 0, *c2, ptr(row_live), ws.data_ptr(), ws_bytes,
                                                stream_ptr()), f"ia_gemm_dgrad_{unit}")
    return out


def gemm_dgrad_rows(dy, w, row_live=None, *, w_kstrided=True, epilogue=EPI_NONE, aux=None, out=None, colsum_out=None):
    """dX[M, N_in] = dy[M, K_out] W (+ EPI_NONE / EPI_ADD / EPI_DGELU_COLSUM); w: [K_out, N_in] (w_kstrided) or its transpose
    [N_in, K_out].  row_live (uint8 [M]) == 0 promises that row of dy (and of aux for EPI_ADD) is all zeros: 32-row blocks without a
    live row are skipped and written as zeros (ia_gemm_dgrad_rows).  row_live=None is gemm(dy, w, b_kstrided=w_kstrided, ...)."""
    return _gemm_dgrad_filtered("rows", dy, w, row_live, w_kstrided, epilogue, aux, out, colsum_out)


def gemm_dgrad_slabs(dy, w, row_live=None, *, w_kstrided=True, epilogue=EPI_NONE, aux=None, out=None):
    """gemm_dgrad_rows (EPI_NONE / EPI_ADD) over the 8-row slabs that hold a live row (ia_gemm_dgrad_slabs); the other slabs' rows are
    written as zeros."""
    return _gemm_dgrad_filtered("slabs", dy, w, row_live, w_kstrided, epilogue, aux, out)


def _gemm_fwd_filtered(unit, x, w, row_live, epilogue, bias, scaled_cols, col_scale, fill, out, pre_out):
    """gemm_fwd_rows (unit "rows": ia_gemm_fwd_rows) and gemm_fwd_slabs ("slabs": ia_gemm_fwd_slabs): one signature, two entry points"""
    lib = _lib.load()
    _need(x, BF16, "x"); _need(w, BF16, "w"); _need(bias, F32, "bias"); _need(row_live, torch.uint8, "row_live")
    M, K = x.shape
    N, Kw = w.shape
    if K != Kw or (row_live is not None and row_live.numel() != M):
        raise ValueError(f"gemm_fwd_{unit}: x, w and row_live do not fit together")
    if out is None:
        out = torch.empty((M, N), device=x.device, dtype=BF16)
    _need(out, BF16, "out")
    if epilogue == EPI_BIAS_GELU and pre_out is None:
        pre_out = torch.empty((M, N), device=x.device, dtype=BF16)
    _need(pre_out, BF16, "pre_out")
    ws_bytes = lib.ia_gemm_slabs_workspace_bytes(M) if unit == "slabs" else lib.ia_gemm_fwd_rows_workspace_bytes(M)
    ws = torch.empty(ws_bytes, device=x.device, dtype=torch.uint8)
    check(getattr(lib, f"ia_gemm_fwd_{unit}")(x.data_ptr(), K, w.data_ptr(), K, out.data_ptr(), N, M, N, K, epilogue, ptr(bias), ptr(pre_out),
                                              scaled_cols, col_scale, ptr(row_live), int(fill), ws.data_ptr(), ws_bytes, stream_ptr()),
          f"ia_gemm_fwd_{unit}")
    if epilogue == EPI_BIAS_GELU:
        return out, pre_out
    return out


def gemm_fwd_rows(x, w, row_live=None, *, epilogue=EPI_NONE, bias=None, scaled_cols=0, col_scale=1.0, fill=True, out=None, pre_out=None):
    """Y[M, N] = x[M, K] w[N, K]^T (+ EPI_NONE / EPI_BIAS with scaled_cols, col_scale / EPI_BIAS_GELU / EPI_BIAS_GELU_ACT = 7) over the
    32-row blocks that hold a live row (row_live uint8 [M]; ia_gemm_fwd_rows).  fill: the other blocks' rows are written as zeros, else
    not written.  row_live=None is the unfiltered call.  EPI_BIAS_GELU returns (out, pre_out)."""
    return _gemm_fwd_filtered("rows", x, w, row_live, epilogue, bias, scaled_cols, col_scale, fill, out, pre_out)


def gemm_fwd_slabs(x, w, row_live=None, *, epilogue=EPI_NONE, bias=None, scaled_cols=0, col_scale=1.0, fill=True, out=None, pre_out=None):
    """gemm_fwd_rows (EPI_NONE / EPI_BIAS with scaled_cols, col_scale / EPI_BIAS_GELU) over the 8-row slabs that hold a live row
    (ia_gemm_fwd_slabs).  fill: the other slabs' rows are written as zeros, else not written.  EPI_BIAS_GELU returns (out, pre_out)."""
    return _gemm_fwd_filtered("slabs", x, w, row_live, epilogue, bias, scaled_cols, col_scale, fill, out, pre_out)


def ln_fwd_rows(x, gamma, beta, eps, row_live, *, bias=None, residual=None, write_z=True, in_place=False, drop_p=0.0, seed=0, stream_id=0):
    """ln_fwd with a row filter (ia_ln_fwd_rows): rows with row_live == 0 read nothing and leave as zeros.  in_place: z is written over x."""
    lib = _lib.load()
    _need(x, BF16, "x"); _need(gamma, F32, "gamma"); _need(beta, F32, "beta"); _need(bias, F32, "bias"); _need(residual, BF16, "residual")
    _need(row_live, torch.uint8, "row_live")
    M, H = x.shape
    y = torch.empty_like(x)
    z = x if in_place else (torch.empty_like(x) if write_z else None)
    mean = torch.empty(M, device=x.device, dtype=F32)
    rstd = torch.empty(M, device=x.device, dtype=F32)
    check(lib.ia_ln_fwd_rows(x.data_ptr(), ptr(bias), ptr(residual), ptr(z), y.data_ptr(), mean.data_ptr(), rstd.data_ptr(),
                             gamma.data_ptr(), ptr(beta), M, H, eps, drop_p, seed, stream_id, ptr(row_live), stream_ptr()), "ia_ln_fwd_rows")
    return y, z, mean, rstd


def ln_fwd(x, gamma, beta, eps, *, bias=None, residual=None, write_z=True, drop_p=0.0, seed=0, stream_id=0):
    lib = _lib.load()
    _need(x, BF16, "x"); _need(gamma, F32, "gamma"); _need(beta, F32, "beta"); _need(bias, F32, "bias"); _need(residual, BF16, "residual")
    M, H = x.shape
    y = torch.empty_like(x)
    z = torch.empty_like(x) if write_z else None
    mean = torch.empty(M, device=x.device, dtype=F32)
    rstd = torch.empty(M, device=x.device, dtype=F32)
    check(lib.ia_ln_fwd(x.data_ptr(), ptr(bias), ptr(residual), ptr(z), y.data_ptr(), mean.data_ptr(), rstd.data_ptr(),
                        gamma.data_ptr(), ptr(beta), M, H, eps, drop_p, seed, stream_id, stream_ptr()), "ia_ln_fwd")
    return y, z, mean, rstd


def ln_bwd(dy, z, mean, rstd, gamma, *, dres=None, dgamma=None, dbeta=None, dbias=None, drop_p=0.0, seed=0, stream_id=0):
    lib = _lib.load()
    _need(dy, BF16, "dy"); _need(z, BF16, "z"); _need(dres, BF16, "dres")
    M, H = dy.shape
    dz = torch.empty_like(dy)
    dx = torch.empty_like(dy) if drop_p > 0 else None
    ws_bytes = lib.ia_ln_bwd_workspace_bytes(M, H)
    ws = torch.empty(ws_bytes, device=dy.device, dtype=torch.uint8)
    check(lib.ia_ln_bwd(dy.data_ptr(), ptr(dres), z.data_ptr(), mean.data_ptr(), rstd.data_ptr(), gamma.data_ptr(), dz.data_ptr(),
                        ptr(dx), ptr(dgamma), ptr(dbeta), ptr(dbias), M, H, drop_p, seed, stream_id, ws.data_ptr(), ws_bytes, 1,
                        stream_ptr()), "ia_ln_bwd")
    return dz, dx


def colsum(x, out, accumulate=True):
    lib = _lib.load()
    _need(x, BF16, "x"); _need(out, F32, "out")
    M, N = x.shape
    ws_bytes = lib.ia_colsum_workspace_bytes(M, N)
    ws = torch.empty(ws_bytes, device=x.device, dtype=torch.uint8)
    check(lib.ia_colsum(x.data_ptr(), N, M, N, out.data_ptr(), int(accumulate), ws.data_ptr(), ws_bytes, stream_ptr()), "ia_colsum")
    return out


def gemm_qscale(a, b, bias, scaled_cols, col_scale):
    """bf16 [M, N] = (a [M, K] @ b [N, K]^T + bias), columns < scaled_cols multiplied by col_scale before the bf16 rounding (the QKV
    projection that hands pre-scaled q to attn_fwd / attn_bwd with q_prescaled=True)"""
    lib = _lib.load()
    _need(a, BF16, "a"); _need(b, BF16, "b"); _need(bias, F32, "bias")
    M, K = a.shape
    N = b.shape[0]
    out = torch.empty((M, N), device=a.device, dtype=BF16)
    check(lib.ia_gemm_bf16_qscale(a.data_ptr(), K, b.data_ptr(), K, out.data_ptr(), N, M, N, K, bias.data_ptr(), scaled_cols, col_scale,
                                  stream_ptr()), "ia_gemm_bf16_qscale")
    return out


def attn_fwd(qkv, B, L, nh, *, key_mask=None, scale=0.125, drop_p=0.0, seed=0, q_prescaled=False):
    """qkv: packed [B*L, 3*nh*64] bf16.  Returns (ctx [B*L, nh*64], lse2 [B, nh, L]).
    q_prescaled: the q columns already hold q * scale * log2(e) (gemm_qscale)"""
    lib = _lib.load()
    _need(qkv, BF16, "qkv"); _need(key_mask, torch.uint8, "key_mask")
    H = nh * 64
    out = torch.empty((B * L, H), device=qkv.device, dtype=BF16)
    lse = torch.empty((B, nh, L), device=qkv.device, dtype=F32)
    base = qkv.data_ptr()
    fn = lib.ia_attn_fwd_ps if q_prescaled else lib.ia_attn_fwd
    check(fn(base, base + 2 * H, base + 4 * H, 3 * H, ptr(key_mask), out.data_ptr(), H, lse.data_ptr(), B, nh, L, scale, drop_p, seed,
             stream_ptr()), "ia_attn_fwd")
    return out, lse


def attn_bwd(qkv, ctx, d_ctx, lse, B, L, nh, *, key_mask=None, scale=0.125, drop_p=0.0, seed=0, dbias=None, q_prescaled=False, return_delta=False,
             masked_rows_dead=False):
    """dbias (fp32 [3H], optional): += column sums of dqkv, i.e. the bias gradient of the fused QKV projection, out of the same launches.
    return_delta: also hand back the [B, nh, L] scratch (the softmax-gradient delta where the dQ / dK,dV kernel pair ran: L > 256 or
    IA_ATTN_EXACT_DELTA=1; the fused backward keeps its key bits there)"""
    lib = _lib.load()
    _need(qkv, BF16, "qkv"); _need(ctx, BF16, "ctx"); _need(d_ctx, BF16, "d_ctx"); _need(lse, F32, "lse")
    H = nh * 64
    dqkv = torch.empty_like(qkv)
    delta = torch.empty((B, nh, L), device=qkv.device, dtype=F32)
    base, dbase = qkv.data_ptr(), dqkv.data_ptr()
    if (q_prescaled or masked_rows_dead) and dbias is None:
        dbias = torch.zeros(3 * H, device=qkv.device, dtype=F32)
    if masked_rows_dead:          # (ia_attn_bwd_bias_ex: d_ctx must be zero at every masked position)
        ws = torch.empty(lib.ia_attn_bwd_bias_workspace_bytes(B, nh, L), device=qkv.device, dtype=torch.uint8)
        check(lib.ia_attn_bwd_bias_ex((1 if q_prescaled else 0) | 2, base, base + 2 * H, base + 4 * H, 3 * H, ptr(key_mask), ctx.data_ptr(),
                                      d_ctx.data_ptr(), H, lse.data_ptr(), delta.data_ptr(), dbase, dbase + 2 * H, dbase + 4 * H, 3 * H,
                                      dbias.data_ptr(), ws.data_ptr(), ws.numel(), B, nh, L, scale, drop_p, seed, stream_ptr()), "ia_attn_bwd_bias_ex")
        return (dqkv, delta) if return_delta else dqkv
    if dbias is not None:
        _need(dbias, F32, "dbias")
        ws = torch.empty(lib.ia_attn_bwd_bias_workspace_bytes(B, nh, L), device=qkv.device, dtype=torch.uint8)
        fn = lib.ia_attn_bwd_bias_ps if q_prescaled else lib.ia_attn_bwd_bias
        check(fn(base, base + 2 * H, base + 4 * H, 3 * H, ptr(key_mask), ctx.data_ptr(), d_ctx.data_ptr(), H, lse.data_ptr(),
                                   delta.data_ptr(), dbase, dbase + 2 * H, dbase + 4 * H, 3 * H, dbias.data_ptr(), ws.data_ptr(), ws.numel(),
                                   B, nh, L, scale, drop_p, seed, stream_ptr()), "ia_attn_bwd_bias")
        return (dqkv, delta) if return_delta else dqkv
    check(lib.ia_attn_bwd(base, base + 2 * H, base + 4 * H, 3 * H, ptr(key_mask), ctx.data_ptr(), d_ctx.data_ptr(), H, lse.data_ptr(),
                          delta.data_ptr(), dbase, dbase + 2 * H, dbase + 4 * H, 3 * H, B, nh, L, scale, drop_p, seed, stream_ptr()),
          "ia_attn_bwd")
    return (dqkv, delta) if return_delta else dqkv


def cast_to_bf16(src, dst=None):
    lib = _lib.load()
    _need(src, F32, "src")
    if dst is None:
        dst = torch.empty(src.shape, device=src.device, dtype=BF16)
    check(lib.ia_cast_f32_to_bf16(src.data_ptr(), dst.data_ptr(), src.numel(), stream_ptr()), "ia_cast_f32_to_bf16")
    return dst


def cast_to_f32(src, dst=None):
    lib = _lib.load()
    _need(src, BF16, "src")
    if dst is None:
        dst = torch.empty(src.shape, device=src.device, dtype=F32)
    check(lib.ia_cast_bf16_to_f32(src.data_ptr(), dst.data_ptr(), src.numel(), stream_ptr()), "ia_cast_bf16_to_f32")
    return dst


# ------------------------------------------------------------------------------------------------ TextCNN tower
def textcnn_taps(sizes, num_filters):
    """(NT, NTP): the tap columns of the projection P and their count rounded up to a multiple of 8 (the leading dimension of P)."""
    nt = num_filters * sum(sizes)
    return nt, (nt + 7) & ~7


def _ptr_array(tensors):
    return (_lib.vp * len(tensors))(*(None if t is None else t.data_ptr() for t in tensors))


def _int_array(values):
    return (_lib.i32 * len(values))(*values)


def textcnn_pack_taps(weights, sizes, taps=None):
    """weights: the fp32 Conv2d weights [F, 2, K, H], one per filter size -> the bf16 tap shadow [2, NTP, H] (include/itemalign.h)."""
    lib = _lib.load()
    for w in weights:
        _need(w, F32, "conv weight")
    F_, H = weights[0].shape[0], weights[0].shape[3]
    if taps is None:
        taps = torch.empty((2, textcnn_taps(sizes, F_)[1], H), device=weights[0].device, dtype=BF16)
    _need(taps, BF16, "taps")
    check(lib.ia_textcnn_pack_taps(_ptr_array(weights), _int_array(sizes), len(sizes), F_, H, taps.data_ptr(), stream_ptr()),
          "ia_textcnn_pack_taps")
    return taps


def textcnn_pool_fwd(P, biases, sizes, B, L, *, p1=0.0, p2=0.0, seed=0, stream_id1=0, stream_id2=0):
    """P [B * L, ldp] fp32 -> (feat [B, NF] fp32, argmax [B, NF] int32)."""
    lib = _lib.load()
    _need(P, F32, "P")
    for b in biases:
        _need(b, F32, "conv bias")
    F_ = biases[0].shape[0]
    feat = torch.empty((B, F_ * len(sizes)), device=P.device, dtype=F32)
    arg = torch.empty((B, F_ * len(sizes)), device=P.device, dtype=torch.int32)
    check(lib.ia_textcnn_pool_fwd(P.data_ptr(), P.shape[1], _ptr_array(biases), _int_array(sizes), len(sizes), F_, B, L, p1, p2, seed,
                                  stream_id1, stream_id2, feat.data_ptr(), arg.data_ptr(), stream_ptr()), "ia_textcnn_pool_fwd")
    return feat, arg


def textcnn_pool_bwd_w(g, arg, x0, x1, sizes, num_filters, L, *, p1=0.0, p2=0.0, seed=0, stream_id1=0, stream_id2=0):
    """-> ([dW_s fp32 [F, 2, K_s, H]], [db_s fp32 [F]])"""
    lib = _lib.load()
    _need(g, F32, "g"); _need(arg, torch.int32, "argmax"); _need(x0, BF16, "x0"); _need(x1, BF16, "x1")
    B, H = g.shape[0], x0.shape[1]
    dW = [torch.empty((num_filters, 2, K, H), device=g.device, dtype=F32) for K in sizes]
    db = [torch.empty(num_filters, device=g.device, dtype=F32) for _ in sizes]
    check(lib.ia_textcnn_pool_bwd_w(g.data_ptr(), arg.data_ptr(), x0.data_ptr(), x1.data_ptr(), _int_array(sizes), len(sizes), num_filters,
                                    B, L, H, p1, p2, seed, stream_id1, stream_id2, _ptr_array(dW), _ptr_array(db), stream_ptr()),
          "ia_textcnn_pool_bwd_w")
    return dW, db


def textcnn_pool_bwd_x(g, arg, weights, sizes, L, *, p1=0.0, p2=0.0, seed=0, stream_id1=0, stream_id2=0):
    """-> dx of channel 0, bf16 [B * L, H]"""
    lib = _lib.load()
    _need(g, F32, "g"); _need(arg, torch.int32, "argmax")
    for w in weights:
        _need(w, F32, "conv weight")
    B, F_, H = g.shape[0], weights[0].shape[0], weights[0].shape[3]
    dx = torch.empty((B * L, H), device=g.device, dtype=BF16)
    check(lib.ia_textcnn_pool_bwd_x(g.data_ptr(), arg.data_ptr(), _ptr_array(weights), _int_array(sizes), len(sizes), F_, B, L, H, p1, p2,
                                    seed, stream_id1, stream_id2, dx.data_ptr(), stream_ptr()), "ia_textcnn_pool_bwd_x")
    return dx


# ------------------------------------------------------------------------------------------------ vocabulary cross-entropy
def vocab_ce_fwd(logits, labels, V=None):
    """nn.CrossEntropyLoss(ignore_index=-1) over logits [M, ld] fp32 (columns V .. ld-1 never read), labels [M] int64 ->
    (lse [M], loss_row [M], loss [2] = (mean over the labelled rows, their count)), all fp32 (ia_vocab_ce_fwd)."""
    lib = _lib.load()
    _need(logits, F32, "logits"); _need(labels, torch.int64, "labels")
    M, ld = logits.shape
    V = ld if V is None else V
    if labels.numel() != M:
        raise ValueError("vocab_ce_fwd: one label per row of logits")
    dev = logits.device
    lse = torch.empty(M, device=dev, dtype=F32)
    loss_row = torch.empty(M, device=dev, dtype=F32)
    loss = torch.empty(2, device=dev, dtype=F32)
    ws_bytes = lib.ia_vocab_ce_workspace_bytes(M)
    ws = torch.empty(max(ws_bytes, 16), device=dev, dtype=torch.uint8)
    check(lib.ia_vocab_ce_fwd(logits.data_ptr(), ld, labels.data_ptr(), lse.data_ptr(), loss_row.data_ptr(), loss.data_ptr(), M, V,
                              ws.data_ptr(), ws_bytes, stream_ptr()), "ia_vocab_ce_fwd")
    return lse, loss_row, loss


def vocab_ce_bwd(logits, labels, lse, loss, dloss, V=None, *, ldg=None, out=None):
    """dlogits bf16 [M, ldg] = (softmax - onehot) * dloss / n_live, zeros in the pad columns and the ignored rows (ia_vocab_ce_bwd).
    dloss: fp32 device scalar; loss: what vocab_ce_fwd returned."""
    lib = _lib.load()
    _need(logits, F32, "logits"); _need(labels, torch.int64, "labels"); _need(lse, F32, "lse"); _need(loss, F32, "loss")
    _need(dloss, F32, "dloss")
    M, ld = logits.shape
    V = ld if V is None else V
    if out is None:
        out = torch.empty((M, (V + 7) & ~7 if ldg is None else ldg), device=logits.device, dtype=BF16)
    _need(out, BF16, "out")
    if labels.numel() != M or lse.numel() != M or out.shape[0] != M or loss.numel() != 2 or dloss.numel() != 1:
        raise ValueError("vocab_ce_bwd: labels, lse and dlogits need one row per row of logits, loss two elements, dloss one")
    check(lib.ia_vocab_ce_bwd(logits.data_ptr(), ld, labels.data_ptr(), lse.data_ptr(), loss.data_ptr(), dloss.data_ptr(), out.data_ptr(),
                              out.shape[1], M, V, stream_ptr()), "ia_vocab_ce_bwd")
    return out


# ------------------------------------------------------------------------------------------------ contrastive loss
def contrastive_fwd(text, image, log_scale):
    """0.5 (CE(sim, arange) + CE(sim^T, arange)), sim = exp(log_scale) text image^T; text, image [B, H] fp32, log_scale a one-element
    fp32 device tensor -> (loss [1], sim [B, B], lse_row [B], lse_col [B]), all fp32 (ia_contrastive_fwd)."""
    lib = _lib.load()
    _need(text, F32, "text"); _need(image, F32, "image"); _need(log_scale, F32, "log_scale")
    B, H = text.shape
    if tuple(image.shape) != (B, H) or log_scale.numel() != 1:
        raise ValueError(f"contrastive_fwd: text {tuple(text.shape)} and image {tuple(image.shape)} must agree, log_scale has one element")
    dev = text.device
    sim = torch.empty((B, B), device=dev, dtype=F32)
    lse_row = torch.empty(B, device=dev, dtype=F32)
    lse_col = torch.empty(B, device=dev, dtype=F32)
    loss = torch.empty(1, device=dev, dtype=F32)
    ws_bytes = lib.ia_contrastive_workspace_bytes(B)
    ws = torch.empty(ws_bytes, device=dev, dtype=torch.uint8)
    check(lib.ia_contrastive_fwd(text.data_ptr(), H, image.data_ptr(), H, log_scale.data_ptr(), sim.data_ptr(), B, lse_row.data_ptr(),
                                 lse_col.data_ptr(), loss.data_ptr(), B, H, ws.data_ptr(), ws_bytes, stream_ptr()), "ia_contrastive_fwd")
    return loss, sim, lse_row, lse_col


def contrastive_bwd(text, image, log_scale, sim, lse_row, lse_col, dloss, *, dlog_scale=None, accumulate=False):
    """-> (dtext [B, H], dimage [B, H], dlog_scale [1]), fp32 (ia_contrastive_bwd).  dloss: fp32 device scalar; sim, lse_row, lse_col: what
    contrastive_fwd returned.  accumulate: add into the given dlog_scale instead of writing it."""
    lib = _lib.load()
    B, H = text.shape
    for t, name in ((text, "text"), (image, "image"), (log_scale, "log_scale"), (sim, "sim"), (lse_row, "lse_row"), (lse_col, "lse_col"), (dloss, "dloss"),
                    (dlog_scale, "dlog_scale")):
        _need(t, F32, name)
    if tuple(image.shape) != (B, H) or tuple(sim.shape) != (B, B) or lse_row.numel() != B or lse_col.numel() != B or dloss.numel() != 1:
        raise ValueError("contrastive_bwd: shapes do not belong to one contrastive_fwd call")
    if accumulate and dlog_scale is None:
        raise ValueError("contrastive_bwd: accumulate needs dlog_scale")
    dev = text.device
    if dlog_scale is None:
        dlog_scale = torch.empty(1, device=dev, dtype=F32)
    dtext = torch.empty((B, H), device=dev, dtype=F32)
    dimage = torch.empty((B, H), device=dev, dtype=F32)
    ws_bytes = lib.ia_contrastive_workspace_bytes(B)
    ws = torch.empty(ws_bytes, device=dev, dtype=torch.uint8)
    check(lib.ia_contrastive_bwd(text.data_ptr(), H, image.data_ptr(), H, log_scale.data_ptr(), sim.data_ptr(), B, lse_row.data_ptr(),
                                 lse_col.data_ptr(), dloss.data_ptr(), dtext.data_ptr(), H, dimage.data_ptr(), H, dlog_scale.data_ptr(),
                                 int(accumulate), B, H, ws.data_ptr(), ws_bytes, stream_ptr()), "ia_contrastive_bwd")
    return dtext, dimage, dlog_scale


def contrastive_shard_fwd(text_l, image_l, text_g, image_g, log_scale, row_offset, world):
    """One rank's part of the contrastive loss of a global batch that `world` ranks share: text_l, image_l [B, H] fp32 are its rows
    row_offset .. row_offset + B - 1 of the gathered text_g, image_g [G, H] -> (loss [1], sim_t [B, G], sim_i [B, G], lse_row_l [B],
    lse_col_l [B]), all fp32 (ia_contrastive_shard_fwd).  The mean of the ranks' losses is contrastive_fwd's of the global batch."""
    lib = _lib.load()
    for t, name in ((text_l, "text_l"), (image_l, "image_l"), (text_g, "text_g"), (image_g, "image_g"), (log_scale, "log_scale")):
        _need(t, F32, name)
    B, H = text_l.shape
    G = text_g.shape[0]
    if tuple(image_l.shape) != (B, H) or tuple(text_g.shape) != (G, H) or tuple(image_g.shape) != (G, H) or log_scale.numel() != 1:
        raise ValueError(f"contrastive_shard_fwd: local {tuple(text_l.shape)} / {tuple(image_l.shape)} and gathered {tuple(text_g.shape)} / "
                         f"{tuple(image_g.shape)} embeddings do not belong together, log_scale has one element")
    dev = text_l.device
    sim_t = torch.empty((B, G), device=dev, dtype=F32)
    sim_i = torch.empty((B, G), device=dev, dtype=F32)
    lse_row_l = torch.empty(B, device=dev, dtype=F32)
    lse_col_l = torch.empty(B, device=dev, dtype=F32)
    loss = torch.empty(1, device=dev, dtype=F32)
    ws_bytes = lib.ia_contrastive_shard_workspace_bytes(B, G)
    ws = torch.empty(ws_bytes, device=dev, dtype=torch.uint8)
    check(lib.ia_contrastive_shard_fwd(text_l.data_ptr(), H, image_l.data_ptr(), H, text_g.data_ptr(), H, image_g.data_ptr(), H,
                                       log_scale.data_ptr(), sim_t.data_ptr(), sim_i.data_ptr(), G, lse_row_l.data_ptr(), lse_col_l.data_ptr(),
                                       loss.data_ptr(), B, G, int(row_offset), int(world), H, ws.data_ptr(), ws_bytes, stream_ptr()),
          "ia_contrastive_shard_fwd")
    return loss, sim_t, sim_i, lse_row_l, lse_col_l


def contrastive_shard_bwd(text_g, image_g, log_scale, sim_t, sim_i, lse_row_g, lse_col_g, dloss, row_offset, world, *, dlog_scale=None,
                          accumulate=False):
    """-> (dtext_l [B, H], dimage_l [B, H], dlog_scale [1]), fp32 (ia_contrastive_shard_bwd): `world` times the rank's share of the
    global-batch gradient.  sim_t, sim_i: what contrastive_shard_fwd returned; lse_row_g, lse_col_g [G]: the lse_row_l / lse_col_l of all
    ranks, gathered like the embeddings; dloss: fp32 device scalar.  accumulate: add into the given dlog_scale instead of writing it."""
    lib = _lib.load()
    G, H = text_g.shape
    for t, name in ((text_g, "text_g"), (image_g, "image_g"), (log_scale, "log_scale"), (sim_t, "sim_t"), (sim_i, "sim_i"),
                    (lse_row_g, "lse_row_g"), (lse_col_g, "lse_col_g"), (dloss, "dloss"), (dlog_scale, "dlog_scale")):
        _need(t, F32, name)
    B = sim_t.shape[0]
    if (tuple(image_g.shape) != (G, H) or tuple(sim_t.shape) != (B, G) or tuple(sim_i.shape) != (B, G) or lse_row_g.numel() != G
            or lse_col_g.numel() != G or dloss.numel() != 1):
        raise ValueError("contrastive_shard_bwd: shapes do not belong to one contrastive_shard_fwd call")
    if accumulate and dlog_scale is None:
        raise ValueError("contrastive_shard_bwd: accumulate needs dlog_scale")
    dev = text_g.device
    if dlog_scale is None:
        dlog_scale = torch.empty(1, device=dev, dtype=F32)
    dtext = torch.empty((B, H), device=dev, dtype=F32)
    dimage = torch.empty((B, H), device=dev, dtype=F32)
    ws_bytes = lib.ia_contrastive_shard_workspace_bytes(B, G)
    ws = torch.empty(ws_bytes, device=dev, dtype=torch.uint8)
    check(lib.ia_contrastive_shard_bwd(text_g.data_ptr(), H, image_g.data_ptr(), H, log_scale.data_ptr(), sim_t.data_ptr(), sim_i.data_ptr(), G,
                                       lse_row_g.data_ptr(), lse_col_g.data_ptr(), dloss.data_ptr(), dtext.data_ptr(), H, dimage.data_ptr(), H,
                                       dlog_scale.data_ptr(), int(accumulate), B, G, int(row_offset), int(world), H, ws.data_ptr(), ws_bytes,
                                       stream_ptr()), "ia_contrastive_shard_bwd")
    return dtext, dimage, dlog_scale
