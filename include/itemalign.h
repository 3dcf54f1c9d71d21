/* itemalign.h — C ABI of libitemalign_hip.so (MI355X / gfx950 kernels of the item-pair matching engine).
 *
 * The reference (sunzeyeah/item-alignment) has no native or FFI boundary: it is pure PyTorch and its
 * arithmetic is dispatched by ATen.  This header therefore *defines* the boundary:
 * each entry point replaces the ATen/cuBLAS work behind one reference call site, cited per function
 * (paths relative to the reference tree).  INTEGRATION.md shows the ctypes stub a maintainer adds.
 *
 * Conventions
 *  - every function returns 0 on success, a negative IA_ERR_* code otherwise (ia_strerror for text);
 *    nothing throws across the boundary.
 *  - all pointers are borrowed DEVICE pointers (tensor.data_ptr()) of contiguous row-major tensors;
 *    nothing is allocated or freed inside; scratch comes in through (workspace, workspace_bytes) with
 *    an ia_*_workspace_bytes query.
 *  - launches are asynchronous on `stream` (pass torch's current HIP stream); no device sync inside.
 *  - "bf16" tensors are passed as void*; fp32 master weights / gradients as float*.
 *  - dropout uses a counter-based generator keyed by (seed, stream_id, element index): forward and
 *    backward of one op must be given the same (drop_p, seed, stream_id).
 */
#ifndef ITEMALIGN_H
#define ITEMALIGN_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct ihipStream_t* ia_stream_t; /* hipStream_t */

#define IA_OK 0
#define IA_ERR_ARG (-1)
#define IA_ERR_LAUNCH (-2)
#define IA_ERR_WORKSPACE (-3)
#define IA_ERR_UNSUPPORTED (-4)

const char* ia_strerror(int code);
/* Bumped whenever an entry point is added or the meaning of an argument / output changes (round 2 changed what IA_EPI_BIAS_GELU
 * stores in C2 and what IA_EPI_DGELU expects in aux): a caller built against another header must not run on this library.
 * item_alignment_amd/_lib.py refuses to load a library whose version differs from the one it was written for. */
#define IA_ABI_VERSION 22
int ia_abi_version(void);

/* ---- GEMM: torch.nn.Linear forward / dgrad / wgrad (src/models/text.py:1241 -> RobertaLayer dense
 * layers; src/models/multimodal.py:811 -> timm Block qkv/proj/fc1/fc2; patch-embed conv as GEMM).
 * C[M,N] = A*B with A k-contiguous ([M,K], lda) or k-strided ([K,M], lda); B k-contiguous ([N,K], ldb;
 * a Linear weight) or k-strided ([K,N], ldb).  epilogue: */
#define IA_EPI_NONE 0
#define IA_EPI_BIAS 1      /* + bias[N] (fp32) */
#define IA_EPI_BIAS_GELU 2 /* x = bf16(acc + bias): C = gelu_erf(x), C2 = gelu_erf'(x) (saved for IA_EPI_DGELU) */
#define IA_EPI_ADD 3       /* + aux[M,N] (bf16, ldaux) */
#define IA_EPI_DGELU 4     /* * aux[M,N], the derivative IA_EPI_BIAS_GELU saved in C2 */
#define IA_EPI_BIAS_ADD 5  /* + bias + aux */
#define IA_EPI_DGELU_COLSUM 6 /* IA_EPI_DGELU, and C2 (fp32 [N]) += column sums of C: the bias gradient of the Linear in front of the GELU
                               * (row-major C with ldc == N; workspace >= ia_gemm_colsum_workspace_bytes(M, N)) */
#define IA_EPI_BIAS_GELU_ACT 7 /* forward-only IA_EPI_BIAS_GELU: C = gelu_erf(bf16(acc + bias)), nothing else is evaluated or stored (ABI 5) */
int ia_gemm_bf16(const void* A, int a_kstrided, int lda, const void* B, int b_kstrided, int ldb, void* C, int c_is_f32, int ldc,
                 int M, int N, int K, int epilogue, const float* bias, const void* aux, int ldaux, void* C2, int accumulate,
                 void* workspace, size_t workspace_bytes, ia_stream_t stream);
/* IA_EPI_BIAS GEMM with k-contiguous operands and bf16 output whose first scaled_cols columns (a multiple of 128) leave as
 * (acc + bias) * col_scale: the fused QKV projection of an encoder layer (RobertaSelfAttention.query/key/value, src/models/text.py:1241;
 * timm Attention.qkv) handing q * softmax scale * log2(e) to the ia_attn_*_ps kernels below -- the division by sqrt(d) of the reference
 * (attention_scores / math.sqrt(head size)) moved in front of the one bf16 rounding of q (ABI 6) */
int ia_gemm_bf16_qscale(const void* A, int lda, const void* B, int ldb, void* C, int ldc, int M, int N, int K, const float* bias,
                        int scaled_cols, float col_scale, ia_stream_t stream);
/* fp32-output (weight-gradient) GEMMs cut K across workgroups when given this much scratch; partial sums are
 * combined in a fixed order (deterministic).  workspace may be NULL (no split).
 * Weight-gradient form (A and B k-strided, fp32 C, IA_EPI_NONE): a non-NULL C2 (fp32 [M]) += sum_k A[k][m], i.e. the bias
 * gradient of the layer whose dW this GEMM computes, out of the same pass over dy (ScaledStdConv2d bias, timm std_conv.py). */
size_t ia_gemm_workspace_bytes(int M, int N, int K, int c_is_f32);
size_t ia_gemm_colsum_workspace_bytes(int M, int N);
/* (ABI 16) The weight gradient of a Linear over padded token rows: dW[N_out, N_in] (+)= dY^T X with dY [M_rows, N_out] (ldy) and
 * X [M_rows, N_in] (ldx), bf16, dW fp32 (ldw) -- ia_gemm_bf16's weight-gradient form (both operands k-strided, IA_EPI_NONE) -- and a row
 * filter like ia_ln_bwd2_rows': row_live [M_rows] uint8 or NULL; row_live[m] == 0 = the caller guarantees that row m of dY is all
 * zeros (a masked position of an encoder whose heads read no masked position, ia_layer_cfg::masked_rows_dead).  A 32-row block of k
 * (rows 32b .. 32b+31) without a live row is then neither fetched nor multiplied (ABI 22; whole 64-row k-tiles before).  Identical results
 * on such inputs (the k-slabs of the split and the order of the reduction do not depend on row_live); a dY that breaks the guarantee loses
 * those rows' products.  NULL = the ia_gemm_bf16 call.  With row_live the workspace (16-byte aligned) holds the split-K partial sums and
 * the block bitmask (ia_kblock_mask, below) and is required: ia_gemm_wgrad_rows_workspace_bytes.  The entry builds the mask and makes the
 * ia_gemm_wgrad_blocks call. */
size_t ia_gemm_wgrad_rows_workspace_bytes(int N_out, int N_in, int M_rows);
/* Diagnostics (tests, tools): 1 when a call of this shape honours row_live or a block mask (outputs large enough for the 256 x 256-tile
 * kernel, whose k loop the filter lives in, and k-slabs of at most 1024 k-tiles), 0 when it reads every row as ia_gemm_bf16 does (the
 * result is the same either way) */
int ia_gemm_wgrad_rows_filters(int N_out, int N_in, int M_rows);
int ia_gemm_wgrad_rows(const void* dY, int ldy, const void* X, int ldx, float* dW, int ldw, int N_out, int N_in, int M_rows,
                       const uint8_t* row_live, int accumulate, void* workspace, size_t workspace_bytes, ia_stream_t stream);
/* The same filter, the mask handed in.  ia_kblock_mask: bit (b & 31) of mask[b >> 5] = OR of row_live over rows 32b .. 32b+31, clipped
 * to M_rows; ia_kblock_mask_bytes(M_rows) bytes; written on the device by one launch, plain stores.  ia_kblock_mask_host is a diagnostic
 * hook: the same words from host memory through the per-block function the device kernel calls (it does not exercise the kernel's ballot
 * and stores).
 * ia_gemm_wgrad_blocks: dW (+)= dY^T X over the 32-row blocks of k whose bit is set -- a block without a live row is neither fetched nor
 * multiplied; the kernel walks the live blocks of each k-slab two to a 64-row k-tile.  Identical results on inputs that keep row_live's
 * guarantee (every fp32 sum keeps its terms and their order).  kblock_mask: device pointer, NULL = the ia_gemm_bf16 call.  The workspace
 * is the split-K one, ia_gemm_workspace_bytes(N_out, N_in, M_rows, 1).  Outputs too small for the 256 x 256-tile kernel, and k-slabs of
 * more than 1024 k-tiles, read every row. */
size_t ia_kblock_mask_bytes(int M_rows);
int ia_kblock_mask(const uint8_t* row_live, int M_rows, uint32_t* mask, ia_stream_t stream);
int ia_kblock_mask_host(const uint8_t* row_live, int M_rows, uint32_t* mask);
int ia_gemm_wgrad_blocks(const void* dY, int ldy, const void* X, int ldx, float* dW, int ldw, int N_out, int N_in, int M_rows,
                         const uint32_t* kblock_mask, int accumulate, void* workspace, size_t workspace_bytes, ia_stream_t stream);
/* The same walk over 16-row steps.  ia_kstep_mask: bit (s & 31) of mask[s >> 5] = OR of row_live over rows 16s .. 16s+15, clipped to
 * M_rows; ia_kstep_mask_bytes(M_rows) bytes; one launch, plain stores; ia_kstep_mask_host: the same words from host memory through the
 * per-step function the device kernel calls (a diagnostic hook, as ia_kblock_mask_host).
 * ia_gemm_wgrad_steps: the twin of ia_gemm_wgrad_blocks over the 16-row steps of k whose bit is set, four to a 64-row k-tile -- a step
 * is one whole MFMA per accumulator, so the results are identical to ia_gemm_wgrad_blocks' and ia_gemm_bf16's on inputs that keep
 * row_live's guarantee.  kstep_mask: device pointer, NULL = the ia_gemm_bf16 call.  The step walk serves k-slabs of at most 512 k-tiles.
 * A longer one takes the block walk from the block mask of the step mask, which the call builds behind the split-K partials (one small
 * launch) when the workspace has ia_gemm_wgrad_rows_workspace_bytes; with the plain split-K workspace such a shape reads every row.
 * ia_gemm_wgrad_walk (diagnostics): the walk a filtered weight gradient of this shape takes given a step mask and that workspace --
 * 2 = 16-row steps, 1 = 32-row blocks, 0 = every row.  The additions did not bump IA_ABI_VERSION: nothing existing changed its meaning. */
size_t ia_kstep_mask_bytes(int M_rows);
int ia_kstep_mask(const uint8_t* row_live, int M_rows, uint32_t* mask, ia_stream_t stream);
int ia_kstep_mask_host(const uint8_t* row_live, int M_rows, uint32_t* mask);
int ia_gemm_wgrad_steps(const void* dY, int ldy, const void* X, int ldx, float* dW, int ldw, int N_out, int N_in, int M_rows,
                        const uint32_t* kstep_mask, int accumulate, void* workspace, size_t workspace_bytes, ia_stream_t stream);
int ia_gemm_wgrad_walk(int N_out, int N_in, int M_rows);
/* (ABI 18) The data gradient of a Linear over padded token rows: dX[M_rows, N_in] = dY[M_rows, K_out] W (+ epilogue), bf16 -- ia_gemm_bf16's
 * data-gradient form (A = dY k-contiguous; B = W [K_out, N_in] k-strided, w_kstrided = 1, or its transposed shadow [N_in, K_out],
 * w_kstrided = 0; epilogue IA_EPI_NONE, IA_EPI_ADD or IA_EPI_DGELU_COLSUM with aux / C2 as there) -- and a row filter.  row_live [M_rows]
 * uint8 or NULL.  Contract: row_live[m] == 0 = the caller guarantees that row m of dY is all zeros and, for IA_EPI_ADD, that row m of aux
 * is all zeros (ia_layer_cfg::masked_rows_dead).  The rows are taken in blocks of 32: a block without a live row is neither fetched nor
 * multiplied, its rows of dX are WRITTEN AS ZEROS (+0; the unfiltered call may give -0 where 0 * gelu' < 0) and they add nothing to the
 * column sums of IA_EPI_DGELU_COLSUM.  Every other element of dX is bit-identical to ia_gemm_bf16's; the column sums add the same fp32
 * terms in another grouping (the per-tile partials cover other rows), so C2 agrees up to fp32 summation order.  NULL = the ia_gemm_bf16
 * call.  With row_live the workspace (32-byte aligned, ia_gemm_dgrad_rows_workspace_bytes: column-sum partials + the block list) is
 * required.  ia_gemm_dgrad_rows_filters: 1 when a call of this shape with contiguous rows (ldy = K_out, ldx = ldaux = N_in) honours
 * row_live (outputs of at least 160 tiles of 256 x 256, every operand below 2 GiB), 0 when it runs every row as ia_gemm_bf16 does (the
 * result is the same either way). */
size_t ia_gemm_dgrad_rows_workspace_bytes(int M_rows, int N_in, int K_out);
int ia_gemm_dgrad_rows_filters(int M_rows, int N_in, int K_out);
int ia_gemm_dgrad_rows(const void* dY, int ldy, const void* W, int w_kstrided, int ldw, void* dX, int ldx, int M_rows, int N_in, int K_out,
                       int epilogue, const void* aux, int ldaux, void* C2, const uint8_t* row_live, void* workspace, size_t workspace_bytes,
                       ia_stream_t stream);
/* the block list itself (int32, ia_row_blocks_bytes(M_rows) bytes, 32-byte aligned), nb = ceil(M_rows / 32), nbr = nb rounded up to 8:
 * list[0] = number of live blocks, list[1] = number of dead blocks, list[2] = nb, list[3..7] = 0; list[8 ..] = the ascending indices of the
 * blocks (rows 32t .. 32t+31, clipped to M_rows) that hold a live row; list[8 + nbr ..] = the ascending indices of the others.  Entries
 * behind either count are unspecified.  ia_row_blocks writes it on the device (one launch, no host synchronisation); ia_row_blocks_host
 * is a diagnostic hook: the same list from host memory through the per-block function the device kernel calls. */
size_t ia_row_blocks_bytes(int M_rows);
int ia_row_blocks(const uint8_t* row_live, int M_rows, int* list, ia_stream_t stream);
int ia_row_blocks_host(const uint8_t* row_live, int M_rows, int* list);
/* Diagnostics (tests, A/B runs): on == 0 makes ia_layer_bwd2 run its data gradients over every row although
 * ia_layer_cfg::masked_rows_dead is set (their lists are withheld; every other row filter stays); returns the previous setting. */
int ia_debug_dgrad_rows(int on);
/* Diagnostics (tests, A/B runs; ABI 19): on == 0 makes ia_layer_fwd / ia_layer_fwd_infer run every row although
 * ia_layer_cfg::masked_rows_dead has IA_ROWS_DEAD_FWD set; returns the previous setting. */
int ia_debug_fwd_rows(int on);
/* (ABI 19) The forward GEMM Y[M_rows, N_out] = X[M_rows, K_in] W[N_out, K_in]^T of ia_gemm_bf16 / ia_gemm_bf16_qscale (both operands
 * k-contiguous, bf16 output; epilogue IA_EPI_NONE, IA_EPI_BIAS with scaled_cols / col_scale, IA_EPI_BIAS_GELU with C2, or
 * IA_EPI_BIAS_GELU_ACT) with a row filter.  row_live [M_rows] uint8 or NULL.  Contract: row_live[m] == 0 = nobody who needs a defined value
 * reads row m of Y / C2 (a padded position under ia_layer_cfg::masked_rows_dead IA_ROWS_DEAD_FWD).  The rows are taken in blocks of 32: a block
 * without a live row is neither fetched nor multiplied.  fill_dead_rows != 0: its rows of Y (and C2) are written as zeros;
 * fill_dead_rows == 0: they are not written at all (they keep what the buffer held).  Every row of a block that holds a live row is
 * bit-identical to the unfiltered call's.  NULL = the unfiltered call.  With row_live the workspace (32-byte aligned,
 * ia_gemm_fwd_rows_workspace_bytes: the block list) is required.  ia_gemm_fwd_rows_filters: 1 when a call of this shape with
 * contiguous rows (ldx = K_in, ldy = N_out) honours row_live, 0 when it runs every row. */
size_t ia_gemm_fwd_rows_workspace_bytes(int M_rows);
int ia_gemm_fwd_rows_filters(int M_rows, int N_out, int K_in);
int ia_gemm_fwd_rows(const void* X, int ldx, const void* W, int ldw, void* Y, int ldy, int M_rows, int N_out, int K_in, int epilogue,
                     const float* bias, void* C2, int scaled_cols, float col_scale, const uint8_t* row_live, int fill_dead_rows,
                     void* workspace, size_t workspace_bytes, ia_stream_t stream);
/* (ABI 20) The same for IA_EPI_BIAS_ADD, Y = X W^T + bias + aux (aux [M_rows, N_out] bf16, ldaux): the fc2 of a pre-LN layer with its
 * residual.  aux is read in the blocks that hold a live row only.  Workspace and the shapes that filter: as ia_gemm_fwd_rows. */
int ia_gemm_fwd_rows_add(const void* X, int ldx, const void* W, int ldw, void* Y, int ldy, int M_rows, int N_out, int K_in, const float* bias,
                         const void* aux, int ldaux, const uint8_t* row_live, int fill_dead_rows, void* workspace, size_t workspace_bytes,
                         ia_stream_t stream);
/* (ABI 20) The group-aligned list: the layout of ia_row_blocks (same size: ia_row_groups_bytes == ia_row_blocks_bytes), the unit of liveness
 * a GROUP of 128 rows (rows 128g .. 128g+127, clipped to M_rows).  The live list holds every 32-row block of every group that holds a live
 * row, ascending -- entries 4i .. 4i+3 are the four blocks of one group; only the last group of M_rows may have fewer -- the dead list the
 * blocks of the other groups.  ia_row_groups_host: the same list from host memory. */
size_t ia_row_groups_bytes(int M_rows);
int ia_row_groups(const uint8_t* row_live, int M_rows, int* list, ia_stream_t stream);
int ia_row_groups_host(const uint8_t* row_live, int M_rows, int* list);
/* (ABI 20) ia_gemm_dgrad_rows' IA_EPI_DGELU_COLSUM form with the 128-row group as the unit: a group without a live row is neither fetched
 * nor multiplied, its rows of dX are written as zeros; every other row of dX is bit-identical to ia_gemm_bf16's, and so is C2: the kernel
 * forms one fp32 column-sum partial per 128-row group, a kept group's partial lands in the slot the unfiltered call gives it and a left-out
 * group's slot holds zeros, which is what its rows (all zeros by the contract) add there.  Contract, workspace
 * (ia_gemm_dgrad_rows_workspace_bytes) and the shapes that filter (ia_gemm_dgrad_rows_filters): as ia_gemm_dgrad_rows. */
int ia_gemm_dgrad_groups_rows(const void* dY, int ldy, const void* W, int w_kstrided, int ldw, void* dX, int ldx, int M_rows, int N_in,
                              int K_out, const void* aux, int ldaux, void* C2, const uint8_t* row_live, void* workspace,
                              size_t workspace_bytes, ia_stream_t stream);
/* (ABI 20, third form) The row filters of ia_gemm_fwd_rows and ia_gemm_dgrad_rows in SLABS of 8 rows (rows 8t .. 8t+7, clipped to
 * M_rows; aligned to multiples of 8 rows of the tensor, never overlapping): a slab without a live row is neither fetched nor multiplied.
 * A padded sequence never lines up with 32-row blocks, so every sequence pays for a partly dead block at its end; in slabs it pays for
 * at most 7 rows.  Every row of a slab that holds a live row is bit-identical to the unfiltered call's.
 * The slab list (ia_row_slabs, ia_row_slabs_host from host memory; ia_row_slabs_bytes, 32-byte aligned): 8 header words -- [0] live
 * slabs, [1] dead slabs, [2] slabs -- then the live slabs, ascending, 32 to an M-tile of the kernel and inside a tile in the order
 * [wave][piece]: the i-th live slab sits at entry (i & ~31) + (i & 3) * 8 + ((i & 31) >> 2), the entries behind the last one of the last
 * tile are -1; then, behind room for every slab rounded up to a multiple of 32, the dead slabs, ascending.
 * ia_gemm_fwd_slabs: epilogue IA_EPI_NONE, IA_EPI_BIAS with scaled_cols / col_scale, or IA_EPI_BIAS_GELU with C2; fill_dead_rows as in
 * ia_gemm_fwd_rows, by slab.  ia_gemm_dgrad_slabs: IA_EPI_NONE or IA_EPI_ADD; the rows of the dead slabs of dX are written as zeros.
 * Other epilogues: IA_ERR_UNSUPPORTED.  row_live == NULL: the unfiltered call.  Workspace with row_live (32-byte aligned):
 * ia_gemm_slabs_workspace_bytes, the list.  The shapes that filter: ia_gemm_fwd_rows_filters / ia_gemm_dgrad_rows_filters; others run
 * every row. */
size_t ia_row_slabs_bytes(int M_rows);
int ia_row_slabs(const uint8_t* row_live, int M_rows, int* list, ia_stream_t stream);
int ia_row_slabs_host(const uint8_t* row_live, int M_rows, int* list);
size_t ia_gemm_slabs_workspace_bytes(int M_rows);
int ia_gemm_fwd_slabs(const void* X, int ldx, const void* W, int ldw, void* Y, int ldy, int M_rows, int N_out, int K_in, int epilogue,
                      const float* bias, void* C2, int scaled_cols, float col_scale, const uint8_t* row_live, int fill_dead_rows,
                      void* workspace, size_t workspace_bytes, ia_stream_t stream);
int ia_gemm_dgrad_slabs(const void* dY, int ldy, const void* W, int w_kstrided, int ldw, void* dX, int ldx, int M_rows, int N_in, int K_out,
                        int epilogue, const void* aux, int ldaux, const uint8_t* row_live, void* workspace, size_t workspace_bytes,
                        ia_stream_t stream);
/* Diagnostics (tests, A/B runs; ABI 20): on == 0 makes the layer calls ignore ia_layer_cfg::out_row_live (every row behind the attention
 * runs under the layer's other filter, as without it); returns the previous setting. */
int ia_debug_out_rows(int on);
/* (ABI 20, second form) The block-packed list: the layout of ia_row_blocks (8 header words, the slots, the dead blocks; the same size)
 * with four slots per wave-row of the remapped kernel, eight per M-tile.  A wave-row holds the live 32-row blocks of one or more WHOLE
 * 128-row groups -- a group's blocks contiguous and ascending, no group across two wave-rows, -1 in the slots behind them; header word 0
 * counts the slots in use (4 x wave-rows).  Groups with 4 live blocks stand alone, each 3 takes a 1, then 2 + 2, an odd 2 with up to two
 * 1s, the remaining 1s by four: a deterministic layout, so the device builder and the _host twin give the same list.  At most
 * 128 x 4096 rows (IA_ERR_UNSUPPORTED beyond).
 * ia_gemm_dgrad_packed: the IA_EPI_DGELU_COLSUM data gradient (as ia_gemm_dgrad_groups_rows, the list handed in) over such a list -- dX
 * on the live blocks, zeros elsewhere, and C2 += the column sums BIT-IDENTICAL to ia_gemm_bf16's on a dY that is zero wherever the list
 * has no block: a lane adds the rows of a group's live blocks in the dense kernel's order with nothing in between, the wave folds and
 * stores at every change of group into that group's slot of the partials, and the second stage is the dense call's.  Workspace:
 * ia_gemm_colsum_workspace_bytes.  A shape the remapped kernel does not serve (ia_gemm_dgrad_rows_filters == 0) runs every row. */
size_t ia_row_groups_packed_bytes(int M_rows);
int ia_row_groups_packed(const uint8_t* row_live, int M_rows, int* list, ia_stream_t stream);
int ia_row_groups_packed_host(const uint8_t* row_live, int M_rows, int* list);
int ia_gemm_dgrad_packed(const void* dY, int ldy, const void* W, int w_kstrided, int ldw, void* dX, int ldx, int M_rows, int N_in, int K_out,
                         const void* aux, int ldaux, void* C2, const int* packed_list, void* workspace, size_t workspace_bytes,
                         ia_stream_t stream);
/* ... on == 0 makes them ignore ia_layer_cfg::out_q_rows (the attention of such a layer runs every query row); returns the previous setting. */
int ia_debug_q_rows(int on);

/* per-launch HIP-event timing of one GEMM instantiation (variant = a_kstrided*1000 + b_kstrided*100 + epilogue*10 + c_is_f32),
 * recorded on the launch stream; used by bench.py for the roofline of the dominant kernel. */
int ia_prof_begin(int variant, int max_launches);
int ia_prof_end(double* total_ms, double* total_flops, int* launches);
double ia_prof_bytes(void); /* algorithmic bytes of the recorded launches: A and B read once, C written once */
/* Diagnostics (ABI 7): occupy `workgroups` whole CUs (one 256-thread workgroup holding all 160 KiB of LDS each, so nothing else can
 * co-reside) for `milliseconds` on `stream` -- a stand-in for a communication kernel that holds CUs next to the persistent GEMMs
 * (tools/cu_contention.py: how much a GEMM on another stream slows down with 0 / 8 / 16 / 32 CUs taken, SURVEY 8(e) overlap of the
 * gradient all-reduce with backward).  With the dynamic tile claim on (ia_debug_gemm_dynamic below) the large persistent GEMM
 * launches take their tiles from one counter per XCD, so a workgroup that starts late finds no work instead of holding a 1/256
 * share back. */
int ia_debug_cu_hog(int workgroups, float milliseconds, ia_stream_t stream);
/* Run-time switch of the dynamic tile claim; returns the previous setting (on < 0: query only).  Default off (static order) unless
 * IA_GEMM_DYNAMIC=1: a host that overlaps a communication stream with the GEMMs (world size > 1) switches it on -- 0-1.5 % per large
 * GEMM for not paying ~1.3-1.5 x when CUs are taken (profiles/r05_cu_contention.txt). */
int ia_debug_gemm_dynamic(int on);

/* ---- LayerNorm tails (RobertaSelfOutput / RobertaOutput: dense -> dropout -> +residual -> LayerNorm;
 * timm Block norm1/norm2).  z = residual + dropout(x + bias); y = LN(z).  z_out may alias x. */
int ia_ln_fwd(const void* x, const float* bias, const void* residual, void* z_out, void* y, float* mean, float* rstd,
              const float* gamma, const float* beta, int M, int H, float eps, float drop_p, uint32_t seed, uint32_t stream_id,
              ia_stream_t stream);
/* (ABI 19) ia_ln_fwd with a row filter: row_live [M] uint8 or NULL (= ia_ln_fwd).  A row with row_live[m] == 0 reads none of its input
 * streams and leaves as zeros in y, in z_out when given (also in place), and in mean / rstd.  Live rows are bit-identical: the dropout
 * stream is indexed by position. */
int ia_ln_fwd_rows(const void* x, const float* bias, const void* residual, void* z_out, void* y, float* mean, float* rstd,
                   const float* gamma, const float* beta, int M, int H, float eps, float drop_p, uint32_t seed, uint32_t stream_id,
                   const uint8_t* row_live, ia_stream_t stream);
size_t ia_ln_bwd_workspace_bytes(int M, int H);
/* dz = LN'(dy) + dres; dx = dropout-masked dz (only when drop_p > 0); dgamma/dbeta/dbias (+)= column sums */
int ia_ln_bwd(const void* dy, const void* dres, const void* z, const float* mean, const float* rstd, const float* gamma, void* dz,
              void* dx, float* dgamma, float* dbeta, float* dbias, int M, int H, float drop_p, uint32_t seed, uint32_t stream_id,
              void* workspace, size_t workspace_bytes, int accumulate, ia_stream_t stream);
/* the same with a second upstream gradient: LayerNorm output gradient = dy + dy2 (dy2 may be NULL; dz may alias dy2).  Replaces the
 * "+ residual gradient" epilogue of the GEMM producing dy in a post-LN layer (transformers RobertaOutput / RobertaSelfOutput backward). */
int ia_ln_bwd2(const void* dy, const void* dy2, const void* dres, const void* z, const float* mean, const float* rstd, const float* gamma,
               void* dz, void* dx, float* dgamma, float* dbeta, float* dbias, int M, int H, float drop_p, uint32_t seed, uint32_t stream_id,
               void* workspace, size_t workspace_bytes, int accumulate, ia_stream_t stream);
/* (round 6, ABI 8) ia_ln_bwd2 with a row filter: row_live [M] uint8 or NULL; row_live[m] == 0 = the caller guarantees that dy, dy2 and dres
 * are zero in row m (a masked position of an encoder whose heads read no masked position, ia_layer_cfg::masked_rows_dead): the row's inputs
 * are not fetched, its dz / dx rows are written as zeros.  Identical results on such inputs; NULL = ia_ln_bwd2. */
int ia_ln_bwd2_rows(const void* dy, const void* dy2, const void* dres, const void* z, const float* mean, const float* rstd,
                    const float* gamma, void* dz, void* dx, float* dgamma, float* dbeta, float* dbias, int M, int H, float drop_p,
                    uint32_t seed, uint32_t stream_id, const uint8_t* row_live, void* workspace, size_t workspace_bytes, int accumulate,
                    ia_stream_t stream);
size_t ia_colsum_workspace_bytes(int M, int N);
int ia_colsum(const void* x, int ld, int M, int N, float* out, int accumulate, void* workspace, size_t workspace_bytes,
              ia_stream_t stream);

/* ---- fused self-attention, head dim 64 (transformers RobertaSelfAttention eager path: QK^T/sqrt(d)
 * + additive key mask -> softmax -> dropout -> PV; timm Attention without mask).  q/k/v point at the
 * first column of head 0 of each operand and share row stride ld_qkv (elements); key_mask is [B,L]
 * uint8 (1 = attend) or NULL; lse2 is [B,nh,L] fp32 (log2-domain log-sum-exp, saved for backward).
 * `delta` of every backward entry point is caller-provided SCRATCH of B*nh*L (general form: B*nh*Lq) floats whose contents after
 * the call are unspecified: the two-kernel path leaves rowsum(dO o O) there, the single-kernel path (32 < L <= 256, Lq == Lk) keeps
 * its attendable-key bit map in it.  Hosts must not read it. */
int ia_attn_fwd(const void* q, const void* k, const void* v, int ld_qkv, const uint8_t* key_mask, void* out, int ld_o, float* lse2,
                int B, int nh, int L, float scale, float drop_p, uint32_t seed, ia_stream_t stream);
int ia_attn_bwd(const void* q, const void* k, const void* v, int ld_qkv, const uint8_t* key_mask, const void* out, const void* d_out,
                int ld_o, const float* lse2, float* delta, void* dq, void* dk, void* dv, int ld_dqkv, int B, int nh, int L,
                float scale, float drop_p, uint32_t seed, ia_stream_t stream);
/* ia_attn_bwd that also returns the bias gradient of the fused QKV projection (reference: the autograd of nn.Linear's bias behind
 * RobertaSelfAttention.query/key/value, src/models/text.py:1241): dbias[3*nh*64] fp32 (q | k | v) += column sums of dq, dk, dv over
 * all tokens, taken in the kernels' epilogues (deterministic two-stage sum); workspace: ia_attn_bwd_bias_workspace_bytes(B, nh, L). */
size_t ia_attn_bwd_bias_workspace_bytes(int B, int nh, int L);
int ia_attn_bwd_bias(const void* q, const void* k, const void* v, int ld_qkv, const uint8_t* key_mask, const void* out, const void* d_out,
                     int ld_o, const float* lse2, float* delta, void* dq, void* dk, void* dv, int ld_dqkv, float* dbias, void* workspace,
                     size_t workspace_bytes, int B, int nh, int L, float scale, float drop_p, uint32_t seed, ia_stream_t stream);

/* The same three on a projection whose q columns were written by ia_gemm_bf16_qscale (q * scale * log2 e, bf16): no kernel scales q again,
 * dq is still the gradient of the unscaled q (what the projection's dgrad / wgrad consume).  `scale` keeps its meaning. (ABI 6) */
int ia_attn_fwd_ps(const void* q, const void* k, const void* v, int ld_qkv, const uint8_t* key_mask, void* out, int ld_o, float* lse2,
                   int B, int nh, int L, float scale, float drop_p, uint32_t seed, ia_stream_t stream);
int ia_attn_bwd_bias_ps(const void* q, const void* k, const void* v, int ld_qkv, const uint8_t* key_mask, const void* out, const void* d_out,
                        int ld_o, const float* lse2, float* delta, void* dq, void* dk, void* dv, int ld_dqkv, float* dbias, void* workspace,
                        size_t workspace_bytes, int B, int nh, int L, float scale, float drop_p, uint32_t seed, ia_stream_t stream);
/* (round 6, ABI 8) the same with flags.  IA_ATTN_MASKED_ROWS_DEAD: the caller guarantees d_out == 0 at every masked position (an
 * encoder whose masked positions never reach the loss -- reference src/models/text.py:1241: RobertaEncoder under an attention mask,
 * heads reading [CLS] / valid spans): the one-kernel backward (L <= 256) skips 32-query blocks that hold only masked positions;
 * dq / dk / dv / dbias are identical to the unflagged call on such inputs. */
#define IA_ATTN_Q_PRESCALED 1
#define IA_ATTN_MASKED_ROWS_DEAD 2
int ia_attn_bwd_bias_ex(int flags, const void* q, const void* k, const void* v, int ld_qkv, const uint8_t* key_mask, const void* out,
                        const void* d_out, int ld_o, const float* lse2, float* delta, void* dq, void* dk, void* dv, int ld_dqkv, float* dbias,
                        void* workspace, size_t workspace_bytes, int B, int nh, int L, float scale, float drop_p, uint32_t seed,
                        ia_stream_t stream);
/* (ABI 20, second form) ia_attn_fwd / ia_attn_fwd_ps and ia_attn_bwd_bias_ex with a query-row limit.  q_rows = n > 0 is the caller's
 * guarantee that nobody reads `out` at query positions >= n of any sequence and that d_out is exactly zero there (a head that reads
 * position 0 only: n = 1).  Forward: only the query tiles that reach in front of n are computed; out and lse2 are bit-identical to the
 * unlimited call in rows < n, and every row the kernel skips is written as zeros (finite whatever the buffer held).  Backward: the
 * 32-query blocks at or beyond n are dead, with or without a key mask -- zero dq rows (+0 where the unlimited call may give -0), nothing
 * for dk / dv; dq, dk, dv and dbias equal the unlimited call's on the same d_out bit for bit.  The backward takes the out / lse2 of a
 * forward with the same limit, a larger one, or none.  q_rows <= 0 or >= L: no limit.  flags: IA_ATTN_Q_PRESCALED (both),
 * IA_ATTN_MASKED_ROWS_DEAD (backward). */
int ia_attn_fwd_q_rows(int flags, const void* q, const void* k, const void* v, int ld_qkv, const uint8_t* key_mask, void* out, int ld_o,
                       float* lse2, int B, int nh, int L, float scale, float drop_p, uint32_t seed, int q_rows, ia_stream_t stream);
int ia_attn_bwd_bias_q_rows(int flags, const void* q, const void* k, const void* v, int ld_qkv, const uint8_t* key_mask, const void* out,
                            const void* d_out, int ld_o, const float* lse2, float* delta, void* dq, void* dk, void* dv, int ld_dqkv,
                            float* dbias, void* workspace, size_t workspace_bytes, int B, int nh, int L, float scale, float drop_p,
                            uint32_t seed, int q_rows, ia_stream_t stream);

/* General form (cross-attention and multi-query attention of the CoCa multimodal layers, src/models/multimodal.py:590-616
 * ParallelTransformerBlock and :665-706 CrossAttention): Lq queries attend to Lk keys per (sequence, head).  q / out /
 * d_out rows are b*Lq + i (strides ld_q, ld_o), k / v rows are b*Lk + j (stride ld_kv), head h at column h*64.  One
 * K/V head shared by all query heads = the nh = 1 case with the query heads folded into rows (q viewed as
 * [B, n*heads, 64], ld_q = 64, Lq = n*heads).  key_mask is [B, Lk] or NULL; lse2 is [B, nh, Lq], delta scratch of the same size
 * (contents unspecified on return, see above). */
int ia_attn_fwd_x(const void* q, int ld_q, const void* k, const void* v, int ld_kv, const uint8_t* key_mask, void* out, int ld_o,
                  float* lse2, int B, int nh, int Lq, int Lk, float scale, float drop_p, uint32_t seed, ia_stream_t stream);
int ia_attn_bwd_x(const void* q, int ld_q, const void* k, const void* v, int ld_kv, const uint8_t* key_mask, const void* out,
                  const void* d_out, int ld_o, const float* lse2, float* delta, void* dq, int ld_dq, void* dk, void* dv, int ld_dkv,
                  int B, int nh, int Lq, int Lk, float scale, float drop_p, uint32_t seed, ia_stream_t stream);
/* (ABI 17) Causal form, the decoder layers of CoCa pre-training (src/models/multimodal.py:529-626 with is_decoding=True): Lq = fold * Lk
 * queries per (sequence, head), query row i attends key j iff j <= i / fold (integer division).  fold = 1 is causal self-attention;
 * the decoder block is nh = 1, fold = heads with the query heads folded into rows.  No key mask and no dropout.  Layouts, lse2
 * [B, nh, Lq] and the delta scratch as for the x form; Lk <= 2048; every pointer 16-byte aligned, every stride a multiple of 8.  The
 * backward adds dk / dv up in a fixed order (no floating-point atomics): two calls on the same inputs give the same bits. */
int ia_attn_fwd_causal_x(const void* q, int ld_q, const void* k, const void* v, int ld_kv, void* out, int ld_o, float* lse2, int B, int nh,
                         int Lk, int fold, float scale, ia_stream_t stream);
int ia_attn_bwd_causal_x(const void* q, int ld_q, const void* k, const void* v, int ld_kv, const void* out, const void* d_out, int ld_o,
                         const float* lse2, float* delta, void* dq, int ld_dq, void* dk, void* dv, int ld_dkv, int B, int nh, int Lk,
                         int fold, float scale, ia_stream_t stream);

/* ---- CoCa multimodal-layer element-wise ops (src/models/multimodal.py:495-524).
 * rotary_split: src rows [M, ld_src] hold q (nh heads x 64) | k (64) | v (64) from column 0 (the head of the fused
 * projection, :586); position = row % n.  q_out [M, nh*64] = rotary(q); kv_out [M, 128] = rotary(k) | v.  The backward
 * call writes (R^T dq | R^T dk | dv) into dsrc[:, 0 : nh*64 + 128].
 * swiglu: src points at 2F columns (x | gate); out [M, F] = silu(gate) * x. */
int ia_rotary_split_fwd(const void* src, int ld_src, void* q_out, void* kv_out, int M, int n, int nh, ia_stream_t stream);
int ia_rotary_split_bwd(const void* dq, const void* dkv, void* dsrc, int ld_src, int M, int n, int nh, ia_stream_t stream);
int ia_swiglu_fwd(const void* src, int ld_src, void* out, int M, int F, ia_stream_t stream);
int ia_swiglu_bwd(const void* dout, const void* src, int ld_src, void* dsrc, int ld_dsrc, int M, int F, ia_stream_t stream);

/* ---- PKGM knowledge-graph rows (src/models/base.py:347-392 RobertaPKGMEmbeddings.kg_embeddings).  ids: [B, ld_ids] int64
 * with the entity id at column ent_col and P relation ids from column rel_lo.  gather: h_sign [B, Dk] = sign(ent[e])
 * (F.normalize over a size-1 dim), r [B*P, Dk] = rel[r_p]; its backward scatters dr into the relation table's gradient
 * (fp32 atomics; the entity table gets none, d sign = 0).  rows: rows[b, row0 + p] = h[b] + r[b, p],
 * rows[b, row0 + P + p] = hp[b] - r[b, p] inside a [B, rows_per_item, H] buffer (hp = proj_mat(h), computed by the
 * caller with ia_linear_small_fwd).  Dk % 4 == 0 (gather forward), H % 4 == 0 (rows forward), 0 <= row0, row0 + 2P <= rows_per_item;
 * sign(+-0) = +0. */
int ia_kg_gather_fwd(const float* ent_table, const float* rel_table, const int64_t* ids, int ld_ids, int ent_col, int rel_lo,
                     float* h_sign, float* r, int B, int P, int Dk, ia_stream_t stream);
int ia_kg_gather_bwd(const float* dr, const int64_t* ids, int ld_ids, int rel_lo, float* rel_grad, int B, int P, int Dk,
                     ia_stream_t stream);
int ia_kg_rows_fwd(const float* h, const float* r, const float* hp, float* rows, int rows_per_item, int row0, int B, int P, int H,
                   ia_stream_t stream);
int ia_kg_rows_bwd(const float* drows, int rows_per_item, int row0, float* dh, float* dr, float* dhp, int B, int P, int H,
                   ia_stream_t stream);

/* ---- vector-similarity head (src/models/base.py:10-34 InnerProduct, :75-88 VecSimClassificationHead.forward) on fp32
 * [B, D] features: sim [B] and the probability it maps to.  measure: */
#define IA_SIM_INNER 0   /* sum(x*y); probs = sigmoid(sim) */
#define IA_SIM_COSINE 1  /* F.cosine_similarity (eps 1e-8); probs = (sim + 1) / 2 */
#define IA_SIM_L1 2      /* F.pairwise_distance p=1 (eps 1e-6 added to the difference); probs = exp(-sim) */
#define IA_SIM_L2 3      /* F.pairwise_distance p=2; probs = exp(-sim) */
int ia_pair_sim_fwd(const float* x, const float* y, float* sim, float* probs, int B, int D, int measure, ia_stream_t stream);
/* dsim / dprobs: upstream gradients of the two outputs (either may be NULL) */
int ia_pair_sim_bwd(const float* x, const float* y, const float* sim, const float* probs, const float* dsim, const float* dprobs,
                    float* dx, float* dy, int B, int D, int measure, ia_stream_t stream);

/* ---- NHWC convolution tower (ECA-NFNet, src/models/image.py:191-199,253-257 -> timm NormFreeNet / NormFreeBlock /
 * ScaledStdConv2d / EcaModule / DownsampleAvg).  Activations are [B, H, W, C] bf16 rows; a standardised weight is
 * what[Cout][k*k*(C/groups)] bf16 with the tap index outermost inside a row (tap = ky*3 + kx).  k = 1 (stride 1,
 * groups 1) is a plain GEMM; k = 3 (stride 1 or 2, padding 1) gathers patches into the workspace and runs one GEMM
 * per group.  C/groups and Cout/groups must be multiples of 8 (the 3-channel stem input is zero-padded to 8). */
int ia_nchw_to_nhwc_bf16(const float* in, void* out, int B, int C, int H, int W, int Cp, ia_stream_t stream);
size_t ia_conv_nhwc_workspace_bytes(int B, int H, int W, int C, int Cout, int k, int stride, int groups);
int ia_conv_nhwc_fwd(const void* x, const void* what, const float* bias, void* y, int B, int H, int W, int C, int Cout, int k, int stride,
                     int groups, void* workspace, size_t workspace_bytes, ia_stream_t stream);
int ia_conv_nhwc_bwd_data(const void* dy, const void* what, void* dx, int B, int H, int W, int C, int Cout, int k, int stride, int groups,
                          void* workspace, size_t workspace_bytes, ia_stream_t stream);
/* dwhat [Cout][k*k*C/groups] fp32 is overwritten; dbias [Cout] (may be NULL) is accumulated.  cols_valid != 0: the workspace
 * is the one ia_conv_nhwc_fwd used for the same x / geometry and still holds its patch matrix (skips the gather). */
int ia_conv_nhwc_bwd_weight(const void* x, const void* dy, float* dwhat, float* dbias, int B, int H, int W, int C, int Cout, int k,
                            int stride, int groups, int cols_valid, void* workspace, size_t workspace_bytes, ia_stream_t stream);
/* ScaledStdConv2d weight: what[o][t*Cgp + c] = (w[o][c][t] - mean_o) * rstd_o * gain[o] * scale (statistics over the
 * Cg*kk fan-in, biased variance taken in two passes about the mean, eps inside the sqrt; channels Cg..Cgp-1 zero; Cgp >= Cg).
 * bwd accumulates into dw / dgain (either may be NULL). */
int ia_ws_conv_weight_fwd(const float* w, const float* gain, void* what, float* mean, float* rstd, int Cout, int Cg, int kk, int Cgp,
                          float scale, float eps, ia_stream_t stream);
int ia_ws_conv_weight_bwd(const float* dwhat, const float* w, const float* gain, const float* mean, const float* rstd, float* dw,
                          float* dgain, int Cout, int Cg, int kk, int Cgp, float scale, ia_stream_t stream);
/* y = silu(x) * scale ; dx = dy * scale * silu'(x) (+ dadd) over n bf16 elements */
int ia_silu_fwd(const void* x, void* y, size_t n, float scale, ia_stream_t stream);
int ia_silu_bwd(const void* dy, const void* x, const void* dadd, void* dx, size_t n, float scale, ia_stream_t stream);
/* the same with a second consumer of y: dx = (dy + dy2) * scale * silu'(x) [+ dadd] -- the SiLU output of a downsampling NormFreeBlock
   feeds conv1 and the projected shortcut (timm nfnet.py NormFreeBlock.forward); replaces autograd's separate gradient add */
int ia_silu_bwd_sum(const void* dy, const void* dy2, const void* x, const void* dadd, void* dx, size_t n, float scale, ia_stream_t stream);
/* AvgPool2d(2, 2, ceil_mode=True, count_include_pad=False) on NHWC */
int ia_avgpool2_fwd(const void* x, void* y, int B, int H, int W, int C, ia_stream_t stream);
int ia_avgpool2_bwd(const void* dy, void* dx, int B, int H, int W, int C, ia_stream_t stream);
/* global average pool [B, HW, C] bf16 -> [B, C] fp32 */
size_t ia_gap_workspace_bytes(int B, int HW, int C);
int ia_gap_fwd(const void* x, float* pooled, int B, int HW, int C, void* workspace, size_t workspace_bytes, ia_stream_t stream);
int ia_gap_bwd(const float* dpooled, void* dx, int B, int HW, int C, ia_stream_t stream);
/* block tail: out = x * sigmoid(conv1d_k(mean_HW x))[b, c] * coef + shortcut (coef = attn_gain * alpha); pooled / gate
 * [B, C] fp32 are saved for ia_eca_bwd, which returns dx (the shortcut's gradient is dout) and accumulates dconv_w [k] */
int ia_eca_fwd(const void* x, const float* conv_w, int k, const void* shortcut, void* out, float* pooled, float* gate, int B, int HW, int C,
               float coef, void* workspace, size_t workspace_bytes, ia_stream_t stream);
/* the same tail with pooled = (mean_HW a) what^T + bias, a [B*HW, Cmid] = the input of the 1x1 convolution (what [C][Cmid] bf16, bias
 * [C] fp32 or NULL) whose output is x: the mean over pixels commutes with the per-pixel linear map, so the reduction reads the narrow
 * tensor (reference src/models/image.py:253-257 -> timm NormFreeBlock.conv3 + attn_last; round 6, ABI 8).  act_out (bf16, same shape as
 * out; may be NULL) = silu(out) * act_scale: the activation the next NormFreeBlock opens with (act1(x) * beta), written by the same
 * pass, bit-identical to ia_silu_fwd(out).  Backward: ia_eca_bwd (+ ia_silu_bwd for the gradient that arrives through act_out). */
size_t ia_eca_fwd_linear_workspace_bytes(int B, int HW, int Cmid);
int ia_eca_fwd_linear(const void* x, const void* a, const void* what, const float* bias, int Cmid, const float* conv_w, int k,
                      const void* shortcut, void* out, void* act_out, float act_scale, float* pooled, float* gate, int B, int HW, int C,
                      float coef, void* workspace, size_t workspace_bytes, ia_stream_t stream);
/* backward of a tail that wrote act_out: dtot = (dact [+ dact2]) * act_scale * silu'(out) [+ dout_direct] (= ia_silu_bwd / ia_silu_bwd_sum,
 * bit for bit) is the whole gradient of out -- returned in dtot, it is also the shortcut's gradient -- and the gate gradient's spatial
 * sums of dtot * x come out of the same pass; dx, dconv_w as ia_eca_bwd.  dact2 / dout_direct may be NULL (round 6, ABI 8). */
int ia_eca_silu_bwd(const void* dact, const void* dact2, const void* out, const void* dout_direct, float act_scale, const void* x,
                    const float* conv_w, int k, const float* pooled, const float* gate, void* dtot, void* dx, float* dconv_w, int B, int HW,
                    int C, float coef, void* workspace, size_t workspace_bytes, ia_stream_t stream);
size_t ia_eca_bwd_workspace_bytes(int B, int HW, int C);
int ia_eca_bwd(const void* dout, const void* x, const float* conv_w, int k, const float* pooled, const float* gate, void* dx,
               float* dconv_w, int B, int HW, int C, float coef, void* workspace, size_t workspace_bytes, ia_stream_t stream);

/* ---- 3x3 stride-1 (grouped) convolution without a patch matrix.  Tensors live on the "padded domain": xp / dxp
 * [B, H+2, W+2, Cin], yp / dyp [B, H+2, W+2, Cout] bf16; inputs (xp, dyp) need a ZERO border, outputs carry garbage in their
 * border rows.  Cin/groups and Cout/groups must be powers of two >= 8.  what [Cout][9 * Cin/groups] (tap-major, as
 * ia_ws_conv_weight_fwd writes it).  Tap t is read as the tensor shifted by (t/3-1)(W+2) + (t%3-1) rows inside the GEMM. */
int ia_conv3x3_padded_fwd(const void* xp, const void* what, const float* bias, void* yp, int B, int H, int W, int Cin, int Cout, int groups,
                          ia_stream_t stream);
int ia_conv3x3_padded_bwd_data(const void* dyp, const void* what, void* dxp, int B, int H, int W, int Cin, int Cout, int groups,
                               ia_stream_t stream);
/* (ABI 7) Direct form for groups of 64 -> 64 channels (every 3x3 convolution of the NF-Net stages) and the stem's 16 -> 32 / 32 -> 64:
 * ia_conv3x3_padded_fwd takes it by itself -- persistent workgroups keep the group's filter bank in LDS and stream 8 x 30-pixel tiles
 * (input with halo staged once by LDS-DMA, the nine taps as LDS row offsets) instead of nine shifted reads per tile through the
 * L2 -> LDS path.  The data gradient is the same kernel on dy with the tap-flipped, transposed bank: ia_conv3x3_flip_weights(what ->
 * what_t [Cin][9 * Cout / groups], the same number of elements), then ia_conv3x3_padded_bwd_data_t.  ia_conv3x3_direct_supported:
 * 1 when forward AND data gradient of the shape take that path.  ia_conv3x3_padded_bwd_weight
 * takes its direct form by itself for the same channel pairs when the launch covers >= 10^5 pixels (transpose reads of the dy and x
 * tiles, one fp32 bank per workgroup, fixed-order fold: bit-reproducible);
 * ia_conv3x3_padded_workspace_bytes covers both forms. */
int ia_conv3x3_direct_supported(int Cin, int Cout, int groups);
int ia_conv3x3_flip_weights(const void* what, void* what_t, int Cin, int Cout, int groups, ia_stream_t stream);
int ia_conv3x3_padded_bwd_data_t(const void* dyp, const void* what_t, void* dxp, int B, int H, int W, int Cin, int Cout, int groups,
                                 ia_stream_t stream);
size_t ia_conv3x3_padded_workspace_bytes(int B, int H, int W, int Cin, int Cout, int groups);
int ia_conv3x3_padded_bwd_weight(const void* xp, const void* dyp, float* dwhat, float* dbias, int B, int H, int W, int Cin, int Cout,
                                 int groups, void* workspace, size_t workspace_bytes, ia_stream_t stream);
/* 3x3 / stride 2 / padding 1 between bordered layouts: xp [B, H+2, W+2, Cin] (zero border) -> yp [B, Ho+2, Wo+2, Cout], Ho = (H-1)/2 + 1
 * (border of yp not written).  The strided convolutions of timm's NormFreeNet (nfnet.py: conv2 of the first block of stages 2-4,
 * 64 channels per group; stem conv4, 64 -> 128) behind reference src/models/image.py:254-257, without a patch matrix: forward = one
 * kernel over the four parity views of x, weight gradient = one kernel over the same views, data gradient = one kernel over the four
 * parity classes of dx.  ia_conv3x3_s2_supported: 1 for Cin = Cout = 64 * groups, or groups = 1, Cin = 64, Cout = 64 n: other shapes go
 * through ia_conv_nhwc_*.  The workspace is the weight gradient's. */
int ia_conv3x3_s2_supported(int Cin, int Cout, int groups);
size_t ia_conv3x3_s2_padded_workspace_bytes(int B, int H, int W, int Cin, int Cout, int groups);
/* y_compact != 0: yp / dyp are [B, Ho, Wo, Cout] without a border (the stem's last convolution feeds compact consumers) */
int ia_conv3x3_s2_padded_fwd(const void* xp, const void* what, const float* bias, void* yp, int B, int H, int W, int Cin, int Cout,
                             int groups, int y_compact, ia_stream_t stream);
int ia_conv3x3_s2_padded_bwd_weight(const void* xp, const void* dyp, float* dwhat, float* dbias, int B, int H, int W, int Cin, int Cout,
                                    int groups, int y_compact, void* workspace, size_t workspace_bytes, ia_stream_t stream);
/* the data gradient (every shape of ia_conv3x3_s2_supported): what_t from
 * ia_conv3x3_flip_weights, dyp bordered with a ZERO border (or compact: y_compact), dxp bordered (interior written).  Cin = Cout = 64 * groups;
 * groups = 1, Cin = 64, Cout = 64 n runs as n launches over the 64-channel slices of dy that add up in dx, what_t then holds n banks
 * (ia_conv3x3_flip_weights(what, what_t, Cout, Cout, n)) */
int ia_conv3x3_s2_padded_bwd_data_t(const void* dyp, const void* what_t, void* dxp, int B, int H, int W, int Cin, int Cout, int groups,
                                    int y_compact, ia_stream_t stream);
/* y = silu(x) * scale between the compact [B,H,W,C] and the zero-bordered [B,H+2,W+2,C] layouts (one flag per side); the
 * backward call produces dx in x's layout from dy in y's layout */
int ia_silu_pad_fwd(const void* x, void* y, int B, int H, int W, int C, float scale, int in_padded, int out_padded, ia_stream_t stream);
int ia_pad_rows(const void* x, void* y, int B, int H, int W, int C, int in_padded, int out_padded, ia_stream_t stream);   /* plain copy */
int ia_silu_pad_bwd(const void* dy, const void* x, void* dx, int B, int H, int W, int C, float scale, int in_padded, int out_padded,
                    ia_stream_t stream);
/* ---- forward-only epilogues (NormFreeNet.embed).  The direct stride-1 / stride-2 kernels with the activation that follows the
 * convolution taken on the fp32 accumulator: y = bf16(silu(acc + bias) * act_scale), one rounding, no pass of its own over the map.
 * Operands as ia_conv3x3_padded_fwd / ia_conv3x3_s2_padded_fwd.  y_compact = 0: y is the bordered [B, Ho + 2, Wo + 2, Cout] domain and
 * only its interior is written -- the border belongs to the caller: a buffer whose border was zeroed once stays a valid zero-bordered
 * input for every later batch; y_compact != 0: y is [B, Ho, Wo, Cout].  Only the direct kernels have this epilogue: a stride-1 channel
 * pair without one (ia_conv3x3_direct_supported's forward half: ci -> co per group in 64->64, 16->32, 32->64, 64->32, 32->16, groups
 * <= 64) and every stride-2 shape outside ia_conv3x3_s2_supported return IA_ERR_UNSUPPORTED before anything is launched.
 * ia_silu_gap_fwd: pooled [B, C] fp32 = scale * mean over HW of silu(x [B, HW, C] bf16), SiLU and sum in fp32 (the tower's tail:
 * final_act + global pool in one read); C % 8 == 0, workspace of ia_gap_workspace_bytes(B, HW, C).  The additions did not bump
 * IA_ABI_VERSION: nothing existing changed its meaning. */
int ia_conv3x3_padded_fwd_act(const void* xp, const void* what, const float* bias, void* y, int B, int H, int W, int Cin, int Cout, int groups,
                              float act_scale, int y_compact, ia_stream_t stream);
int ia_conv3x3_s2_padded_fwd_act(const void* xp, const void* what, const float* bias, void* y, int B, int H, int W, int Cin, int Cout,
                                 int groups, float act_scale, int y_compact, ia_stream_t stream);
int ia_silu_gap_fwd(const void* x, float* pooled, int B, int HW, int C, float scale, void* workspace, size_t workspace_bytes,
                    ia_stream_t stream);

/* ---- pre-activation ResNetV2 tower pieces (reference src/models/image.py:298-378 ResNetTwoTower -> timm 0.6.5 resnetv2.py
 * with norm_layer=BatchNormAct2d; README.md:187-197 `--model_name resnetv2_50`).  NHWC rows [B*H*W, C] bf16 as above. */
/* BatchNorm2d + ReLU.  The rows are `segments` equal consecutive runs, each normalised with its own batch statistics (the
 * reference runs the two towers as two forward calls: image.py:337-341).  training: batch statistics, running_mean/var [C]
 * (NULL allowed) updated with `momentum` segment by segment; else the running statistics are used.  mean / rstd
 * [segments][C] fp32 are saved for the backward call. */
size_t ia_bn_act_workspace_bytes(int rows, int C, int segments);
int ia_bn_act_fwd(const void* x, const float* gamma, const float* beta, float* running_mean, float* running_var, void* y, float* mean,
                  float* rstd, int rows, int C, int segments, float eps, float momentum, int training, int relu, void* workspace,
                  size_t workspace_bytes, ia_stream_t stream);
/* dx (+ extra [rows, C] bf16 when not NULL: a second gradient reaching x), dgamma / dbeta [C] accumulated (NULL allowed) */
int ia_bn_act_bwd(const void* dy, const void* x, const float* gamma, const float* beta, const float* mean, const float* rstd,
                  const void* extra, void* dx, float* dgamma, float* dbeta, int rows, int C, int segments, int training, int relu,
                  void* workspace, size_t workspace_bytes, ia_stream_t stream);
/* GroupNorm(groups, C, eps) + ReLU: the norm layer of the BiT towers (`--model_name resnetv2_50x3_bitm_in21k`, named by the help text
 * of finetune_image.py:23 and handed to timm at :191; timm 0.6.5 resnetv2.py norm_layer=GroupNormAct(num_groups=32)).  x: `images`
 * images of rows / images pixels each; biased statistics per (image, group of C / groups consecutive channels), the same in training
 * and eval mode.  mean / rstd [images][C] fp32 (the group's value once per channel) are saved for the backward call. */
size_t ia_gn_act_workspace_bytes(int rows, int C, int images);
int ia_gn_act_fwd(const void* x, const float* gamma, const float* beta, void* y, float* mean, float* rstd, int rows, int C, int images,
                  int groups, float eps, int relu, void* workspace, size_t workspace_bytes, ia_stream_t stream);
/* dx (+ extra [rows, C] bf16 when not NULL), dgamma / dbeta [C] accumulated (NULL allowed) */
int ia_gn_act_bwd(const void* dy, const void* x, const float* gamma, const float* beta, const float* mean, const float* rstd,
                  const void* extra, void* dx, float* dgamma, float* dbeta, int rows, int C, int images, int groups, int relu,
                  void* workspace, size_t workspace_bytes, ia_stream_t stream);
/* cols [B*Ho*Wo, Kp] bf16: patch matrix of a k x k / stride / pad convolution read from NCHW fp32 images; column
 * (ky*k + kx)*C + c, columns >= k*k*C zero, Kp % 8 == 0 (the 7x7 stem, timm resnetv2.py create_resnetv2_stem) */
int ia_patches_nchw(const float* images, void* cols, int B, int C, int H, int W, int k, int stride, int pad, int Kp, ia_stream_t stream);
/* MaxPool2d(3, stride 2, padding 1): y [B*Ho*Wo, C] bf16, arg [B*Ho*Wo, C] u8 = window position of the first maximum */
int ia_maxpool3s2_fwd(const void* x, void* y, uint8_t* arg, int B, int H, int W, int C, ia_stream_t stream);
/* pad_zero != 0: window positions outside the image count as zeros -- ConstantPad2d(1, 0.) + MaxPool2d(3, 2, padding 0), the 'fixed'
 * stem of the BiT towers (timm resnetv2.py create_resnetv2_stem); ia_maxpool3s2_bwd serves both forms */
int ia_maxpool3s2_fwd_ex(const void* x, void* y, uint8_t* arg, int B, int H, int W, int C, int pad_zero, ia_stream_t stream);
int ia_maxpool3s2_bwd(const void* dy, const uint8_t* arg, void* dx, int B, int H, int W, int C, ia_stream_t stream);
/* rows read by a strided 1x1 convolution: y [B*Ho*Wo, C] = x[b, oy*stride, ox*stride, :]; the backward call writes
 * dx = base (NULL = zeros; may alias dx) + dy scattered onto the stride grid */
int ia_rows_subsample_fwd(const void* x, void* y, int B, int H, int W, int C, int stride, ia_stream_t stream);
int ia_rows_subsample_bwd(const void* dy, const void* base, void* dx, int B, int H, int W, int C, int stride, ia_stream_t stream);
/* plain convolution weight: what [Cout][ldw] bf16 (tap-major, channels padded to Cgp, row padded with zeros to ldw) from the
 * PyTorch layout w [Cout][Cg][kk] fp32; the grad call does dw += dwhat in the inverse mapping */
int ia_conv_weight_pack(const float* w, void* what, int Cout, int Cg, int kk, int Cgp, int ldw, ia_stream_t stream);
int ia_conv_weight_unpack_grad(const float* dwhat, float* dw, int Cout, int Cg, int kk, int Cgp, int ldw, ia_stream_t stream);

/* ---- image input pipeline on the GPU (src/data/data.py:838-866: timm create_transform(is_training=False) = PIL bicubic
 * resize -> ToTensor -> Normalize).  ia_resize_pass_u8 is one separable pass of Pillow's 8-bit resampler (Resample.c) over
 * a batch of equally sized uint8 RGB frames: horizontal != 0: src [B, other_len, in_len, 3] -> dst [B, other_len, out_len, 3];
 * else src [B, in_len, other_len, 3] -> dst [B, out_len, other_len, 3].  bounds [out_len][2] (first tap, tap count) and
 * coeffs [out_len][ksize] (int32, 8.22 fixed point) are Pillow's precompute_coeffs / normalize_coeffs_8bpc tables, built
 * by the host (item_alignment_amd/data/gpu_preproc.py): results are bit-identical to Image.resize(size, BICUBIC). */
int ia_resize_pass_u8(const uint8_t* src, uint8_t* dst, const int* bounds, const int* coeffs, int ksize, int B, int in_len, int out_len,
                      int other_len, int horizontal, ia_stream_t stream);
/* The same pass with an explicit source layout for the horizontal pass (rows src_pitch_bytes apart, frames src_frame_bytes apart): a
 * RandomResizedCrop window of a decoded frame is the frame's own pitch with src at the window's first pixel and in_len = the window
 * width; out_len may be the CenterCrop sub-range of a resize when bounds / coeffs are the matching slice of the tables (timm
 * create_transform as the reference calls it, src/data/data.py:838-841; torchvision on PIL images -> Pillow Resample.c). */
int ia_resize_pass_u8_ex(const uint8_t* src, size_t src_pitch_bytes, size_t src_frame_bytes, uint8_t* dst, const int* bounds,
                         const int* coeffs, int ksize, int B, int in_len, int out_len, int other_len, int horizontal, ia_stream_t stream);
/* One step of torchvision ColorJitter (= Pillow ImageEnhance.{Brightness,Contrast,Color}: Image.blend(degenerate, image, factor),
 * Blend.c float arithmetic) on uint8 frames [B,H,W,3] in place.  op [B] int32: 0 none, 1 brightness, 2 contrast, 3 saturation;
 * factor [B] fp32; scratch: B x 8 bytes of device memory (contrast means); any_contrast != 0 when some op[b] == 2.  One call per
 * position of the images' random op order (reference --color_jitter, data.py:841). */
int ia_color_jitter_step_u8(uint8_t* frames, const int* op, const float* factor, void* scratch, int B, int H, int W, int any_contrast,
                            ia_stream_t stream);
/* uint8 [B,S0,S1,3] -> fp32 [B,3,S0,S1] = (x/255 - mean)/std with IEEE fp32 division (ToTensor + Normalize), optional
 * per-image horizontal flip (flip: [B] device bytes or NULL); mean3 / std3: HOST arrays of 3 floats */
int ia_u8_to_nchw_normalized(const uint8_t* src, const uint8_t* flip, float* out, int B, int S0, int S1, const float* mean3,
                             const float* std3, ia_stream_t stream);

/* ---- baseline JPEG decode on the GPU (--gpu_jpeg; the reference decodes with PIL inside __getitem__, src/data/data.py:848-860).  The
 * host (item_alignment_amd/data/jpeg.py) parses the headers, removes the stuffed zeros and cuts the scan at its restart markers; the
 * two stages below turn a batch of such scans into the uint8 [H, W, 3] frames Pillow produces, byte for byte.
 * Layouts (all built by data/jpeg.py): desc [n_images][16] int32 = W, H, components (1 or 3), luma sampling h, v, MCUs per row,
 * MCU rows, MCUs per restart segment, segments, first segment (index into the seg_* arrays), pieces, first piece, pieces of the
 * longest segment, first coefficient (int16 elements), first plane byte, first output byte.  scan: the unstuffed segments, each at a
 * multiple of 4 bytes; seg_off / seg_len: byte offset / length per segment; seg_piece0: image-local index of a segment's first piece;
 * piece_seg: image-local segment per piece; tables [n_images][6][1424]: per component a DC and an AC Huffman table (512 x uint16
 * 9-bit look-ahead, int32 maxcode[18], int32 valoff[17], 256 symbols); qt [n_images][3][64] bytes in natural order.
 * Coefficients: per image the component grids (block raster over the MCU-padded grid, 64 natural-order int16 per block, DC summed)
 * with 64 untouched elements in front of, between and behind them.
 * ia_jpeg_entropy: scan -> coefficients.  subseq_bits (multiple of 32, >= 64) is the piece length; piece_ws = 10 * total_pieces
 * int32 of scratch.  status[i] != 0: image i did not decode (a code matched nothing, a zigzag index passed 63, or the bits ran out
 * before the blocks); rounds[i]: synchronisation rounds used.  One launch.
 * ia_jpeg_reconstruct: coefficients -> RGB (dequantisation, libjpeg's accurate integer IDCT, fancy upsampling, 16.16 YCbCr -> RGB).
 * planes: scratch, one byte per coefficient.  Two launches, n_images <= 65535. */
int ia_jpeg_entropy(const int* desc, int n_images, const uint8_t* scan, const int* seg_off, const int* seg_len, const int* seg_piece0,
                    const int* piece_seg, const uint8_t* tables, int* piece_ws, int total_pieces, int16_t* coef, int subseq_bits,
                    int* status, int* rounds, ia_stream_t stream);
int ia_jpeg_reconstruct(const int* desc, int n_images, const int16_t* coef, const uint8_t* qt, uint8_t* planes, uint8_t* out,
                        ia_stream_t stream);

/* ---- embeddings (src/models/base.py:238-279, :501-556, :394-442).  0 < H <= 4096, H % 8 == 0; extra_idx (may be NULL) needs extra;
 * z_out = bf16(word|extra + type + pos), mean / rstd are the statistics of that rounded z.  The backward call returns IA_ERR_WORKSPACE
 * for a workspace below ia_embed_ln_bwd_workspace_bytes(M, H). */
int ia_embed_ln_fwd(const int64_t* ids, const int64_t* type_ids, const int64_t* pos_ids, const int32_t* extra_idx, const float* word,
                    const float* type, const float* pos, const float* extra, const float* gamma, const float* beta, void* z_out,
                    void* y, float* mean, float* rstd, int M, int H, float eps, float drop_p, uint32_t seed, uint32_t stream_id,
                    ia_stream_t stream);
size_t ia_embed_ln_bwd_workspace_bytes(int M, int H);
int ia_embed_ln_bwd(const void* dy, const void* z, const float* mean, const float* rstd, const float* gamma, const int64_t* ids,
                    const int64_t* type_ids, const int64_t* pos_ids, const int32_t* extra_idx, const int32_t* row_order,
                    const int32_t* word_order, const int32_t* pos_order, const int32_t* type_order, float* dword, float* dtype, float* dpos, float* dextra, float* dgamma, float* dbeta, int M, int H, int L, int word_pad, int pos_pad,
                    float drop_p, uint32_t seed, uint32_t stream_id, void* workspace, size_t workspace_bytes, ia_stream_t stream);
/* row_order (int32 [M], may be NULL): the rows sorted by position id, for unpadded token rows that have no [M/L, L] grid — the
 * position / token-type gradients are then run-length accumulated along that list instead of down the columns of the grid.
 * word_order / pos_order / type_order (int32 [M], required with dword / dpos / dtype): the rows stably sorted by the table row they
 * add to (-1 = none: extra rows and word_pad rows for the word table, pos_pad rows for the position table, first).  Each table row
 * is summed over its input rows in that order, so the table gradients are the same from run to run. */

/* ---- ViT input side (timm PatchEmbed + cls token + pos_embed; src/models/multimodal.py:811).  im2col: P % 8 == 0, S % P == 0, patch
 * column = (c, ph, pw).  tokens: H > 0, H % 8 == 0. */
int ia_im2col_patch(const float* images, void* patches, int B, int C, int S, int P, ia_stream_t stream);
int ia_vit_tokens_fwd(const void* patch, const float* cls, const float* pos, void* tokens, int B, int NP, int H, ia_stream_t stream);
int ia_vit_tokens_bwd(const void* dtokens, void* dpatch, float* dcls, float* dpos, int B, int NP, int H, int accumulate,
                      ia_stream_t stream);

/* ---- CLS row pick with dropout (features[:, 0, :] -> dropout, src/models/base.py:104,140-141).  src / dsrc rows are ld elements apart
 * (ld >= H, any H > 0); the dropout element index is b * H + col; the backward call needs distinct rows. */
int ia_gather_rows_fwd(const void* src, int ld, const int32_t* rows, float* out, int B, int H, float drop_p, uint32_t seed,
                       uint32_t stream_id, ia_stream_t stream);
int ia_gather_rows_bwd(const float* dout, int ld, const int32_t* rows, void* dsrc, int B, int H, float drop_p, uint32_t seed,
                       uint32_t stream_id, int accumulate, ia_stream_t stream);

/* ---- heads and loss (src/models/base.py:103-117, :139-157; nn.CrossEntropyLoss text.py:1292) */
#define IA_ACT_NONE 0
#define IA_ACT_TANH 1
int ia_linear_small_fwd(const float* x, int ldx, const float* W, const float* bias, float* y, int B, int N, int K, int act,
                        ia_stream_t stream);
int ia_linear_small_bwd(const float* dy, const float* y, const float* x, int ldx, const float* W, float* dx, int lddx, float* dW,
                        float* db, int B, int N, int K, int act, ia_stream_t stream);
int ia_pair_head_ce_fwd(const float* x, const float* y, const float* W, const float* bias, const int64_t* labels, float* logits,
                        float* probs, float* loss, float* loss_per, int B, int D, int C, ia_stream_t stream);
int ia_pair_head_ce_bwd(const float* probs, const int64_t* labels, const float* dloss, const float* x, const float* y, const float* W,
                        float* dx, float* dy, float* dW, float* db, int B, int D, int C, ia_stream_t stream);

/* span means of the auxiliary attribute-pair task (reference text.py:66-102 AuxiliaryTaskPair: mean of the token rows of a
 * key:value span, for the source and the target item; the pair head + CE above finishes it).  spans [S][2] int32 = absolute
 * (first row, end row) into seq [rows, ld] bf16; out [S][H] fp32.  Backward: dseq [B*L, H] bf16 overwritten; span_ptr [B+1]
 * delimits the spans of each sample.  H > 0, H % 8 == 0, ld % 8 == 0. */
int ia_span_mean_fwd(const void* seq, int ld, const int* spans, float* out, int S, int H, ia_stream_t stream);
int ia_span_mean_bwd(const float* dout, const int* spans, const int* span_ptr, void* dseq, int B, int L, int H, ia_stream_t stream);

/* packed ("unpadded") self-attention: rows of all sequences back to back, sequence b = rows cu_seqlens[b] .. cu_seqlens[b+1]
 * (int32 [B+1], device; total_tokens = cu_seqlens[B]); q / k / v share the row stride ld_qkv; no key mask; lse2 / delta stay
 * [B, nh, Lmax] with Lmax the longest sequence.  Same arithmetic as ia_attn_fwd / ia_attn_bwd on the valid tokens. */
int ia_attn_fwd_varlen(const void* q, const void* k, const void* v, int ld_qkv, const int* cu_seqlens, int total_tokens, void* out, int ld_o,
                       float* lse2, int B, int nh, int Lmax, float scale, float drop_p, uint32_t seed, ia_stream_t stream);
int ia_attn_bwd_varlen(const void* q, const void* k, const void* v, int ld_qkv, const int* cu_seqlens, int total_tokens, const void* out,
                       const void* d_out, int ld_o, const float* lse2, float* delta, void* dq, void* dk, void* dv, int ld_dqkv, int B, int nh,
                       int Lmax, float scale, float drop_p, uint32_t seed, ia_stream_t stream);

int ia_attn_fwd_varlen_ps(const void* q, const void* k, const void* v, int ld_qkv, const int* cu_seqlens, int total_tokens, void* out, int ld_o,
                          float* lse2, int B, int nh, int Lmax, float scale, float drop_p, uint32_t seed, ia_stream_t stream);
int ia_attn_bwd_varlen_ps(const void* q, const void* k, const void* v, int ld_qkv, const int* cu_seqlens, int total_tokens, const void* out,
                          const void* d_out, int ld_o, const float* lse2, float* delta, void* dq, void* dk, void* dv, int ld_dqkv, int B, int nh,
                          int Lmax, float scale, float drop_p, uint32_t seed, ia_stream_t stream);

/* ---- optimiser (torch.optim.AdamW, finetune_multimodal.py:296-308,460-468) */
/* dst[offset + c*rows + r] = src[offset + r*cols + c] for each of the n table entries {offset_lo, offset_hi, rows, cols} (uint32 x 4,
 * device memory; element offsets, the same in src and dst): the transposed weight shadows of ia_layer_weights::wt_*.  (ABI 7) */
int ia_transpose_bf16_batched(const void* src, void* dst, const void* table, int n, int max_tiles, ia_stream_t stream);
int ia_adamw_flat(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, void* shadow_bf16, const void* chunk_table,
                  int n_chunks, float lr, float beta1, float beta2, float eps, float weight_decay, int step, float grad_scale,
                  ia_stream_t stream);
/* LAMB (You et al., ICLR 2020) over the same five arenas (a pure addition: the ABI version is unchanged).  With t = step >= 1:
 *   s = grad_scale                                                             if max_grad_norm <= 0
 *     = grad_scale * min(1, max_grad_norm / (grad_scale * ||g||_2 + 1e-6))     otherwise (||g|| over every chunk of the table)
 *   g' = s g;  m = b1 m + (1 - b1) g';  v = b2 v + (1 - b2) g'^2
 *   u  = (m / (1 - b1^t)) / (sqrt(v / (1 - b2^t)) + eps) + wd w          wd = weight_decay where the chunk's decay word is set, else 0
 *   r_T = ||w_T||_2 / ||u_T||_2 if the tensor has IA_LAMB_ADAPT and both norms are > 0, else 1  (w before the update; no clamp)
 *   w  = w - lr r_T u;  shadow = bf16(w), round to nearest even (shadow_bf16 may be NULL)
 * chunk_table: as for ia_adamw_flat (n_chunks x {offset_lo, offset_hi, count <= 4096, decay}, offsets 4-element aligned).
 * tensor_table: n_tensors x {first_chunk, n_chunks, flags} (uint32 x 3, device memory): the chunks of one tensor are adjacent and
 * ascending in chunk_table; every chunk belongs to exactly one tensor (a chunk no tensor claims is stepped with r = 1).  Elements
 * outside the chunks (alignment padding, frozen tensors) are neither read nor written.
 * Three launches on `stream` (five with clipping), no host synchronisation, nothing read back, no atomics: partial sums are fp32 inside
 * a chunk and combined in fp64 in an order fixed by the tables, so equal inputs give equal bits on every run and every rank.
 * workspace: >= ia_lamb_workspace_bytes(n_chunks, n_tensors), 16-byte aligned; after the step the float at byte 16 + 4 i is r_T of
 * tensor i.  IA_ERR_ARG: a null pointer, n_chunks / n_tensors / step <= 0; IA_ERR_WORKSPACE: workspace null, small or misaligned. */
#define IA_LAMB_ADAPT 1
size_t ia_lamb_workspace_bytes(int n_chunks, int n_tensors);
int ia_lamb_flat(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, void* shadow_bf16, const void* chunk_table,
                 int n_chunks, const void* tensor_table, int n_tensors, float lr, float beta1, float beta2, float eps, float weight_decay,
                 int step, float grad_scale, float max_grad_norm, void* workspace, size_t workspace_bytes, ia_stream_t stream);
int ia_cast_f32_to_bf16(const float* src, void* dst, size_t n, ia_stream_t stream);
int ia_cast_bf16_to_f32(const void* src, float* dst, size_t n, ia_stream_t stream);

/* ---- knowledge-graph pretraining (pkgm_pretrain.py: torchkge PKGMModel / TransEModel scoring, MarginLoss, BernoulliNegativeSampler,
 * Trainer + torch.optim.Adam with coupled L2; ABI 12).  fp32 tables, projection and gradients; ids int64.
 * ia_kgpt_score runs B positive triples (h, t, r) and B negatives (nh, nt, r): hn = normalize(ent[h]), tn = normalize(ent[t]),
 * score = -d(hn + rel[r], tn) - d(hn P^T, rel[r]) (the second term only when proj != NULL: PKGM; TransE passes NULL), d = |.|_2^2
 * (norm 2) or |.|_1 (norm 1).  mode IA_KGPT_SCORE: pos / neg only.  IA_KGPT_GRAD: and the gradients of sum(dpos * pos + dneg * neg).
 * IA_KGPT_MARGIN: and loss[0] = sum max(0, margin - pos + neg) with its gradients.  Gradients ACCUMULATE (+=) into dent [n_ent, D],
 * drel [n_rel, D] and dproj [D, D]; ent_order is the stable sort of the 4B entity keys (h | nh | t | nt) by value, rel_order that of the
 * 2B relation keys (r | r): every table row is the sum of its contributions in that order, so the gradients are bit-identical from run
 * to run.  workspace >= ia_kgpt_workspace_bytes(B, D, proj != NULL). */
#define IA_KGPT_SCORE 0
#define IA_KGPT_GRAD 1
#define IA_KGPT_MARGIN 2
size_t ia_kgpt_workspace_bytes(int B, int D, int use_proj);
int ia_kgpt_score(const float* ent, const float* rel, const float* proj, const int64_t* h, const int64_t* t, const int64_t* r,
                  const int64_t* nh, const int64_t* nt, int B, int D, int n_ent, int n_rel, int norm, int mode, float margin,
                  const float* dpos, const float* dneg, float* pos, float* neg, float* loss, const int32_t* ent_order, const int32_t* rel_order,
                  float* dent, float* drel, float* dproj, void* workspace, size_t workspace_bytes, ia_stream_t stream);
/* torch.optim.Adam step with coupled L2 (g += weight_decay * p) over n contiguous fp32 values (16-byte aligned); the gradient is set
 * to zero in the same pass.  step counts from 1.  (ia_adamw_flat is the decoupled AdamW of the fine-tuning path.) */
int ia_kgpt_adam_l2(float* params, float* grads, float* exp_avg, float* exp_avg_sq, size_t n, float lr, float beta1, float beta2,
                    float eps, float weight_decay, int step, ia_stream_t stream);
/* x[i, :] /= max(|x[i, :]|_2, 1e-12) in place (PKGMModel.normalize_parameters) */
int ia_kgpt_row_normalize(float* x, int rows, int D, ia_stream_t stream);
/* one negative per fact: head replaced with probability bern_probs[r] (0.5 for r outside [0, n_probs)), the tail otherwise, by an id
 * uniform in [1, n_ent); counter-based generator keyed by (seed, fact index) */
int ia_kgpt_corrupt(const int64_t* h, const int64_t* t, const int64_t* r, int n, const float* bern_probs, int n_probs, int n_ent,
                    uint64_t seed, int64_t* nh, int64_t* nt, ia_stream_t stream);
/* Link-prediction ranks (torchkge LinkPredictionEvaluator; ABI 13).  One call ranks B queries on one side over the raw tables (no
 * normalisation, no projection term: PKGM and TransE rank alike).  IA_KGPT_LP_TAIL: q = ent[h] + rel[r], true entity t;
 * IA_KGPT_LP_HEAD: q = ent[t] - rel[r], true entity h.  d(q, c) = sum_k (q_k - c_k)^2 (norm 2) or sum_k |q_k - c_k| (norm 1), one fp32
 * accumulator per pair summed in k order; score = -d.  rank[b] = 1 + #{c != true : d_c <= d_true} over all n_ent candidates (int64,
 * ties count against the query).  Filter: grp_off [n_grp + 1] / grp_ids (int64 CSR, each group a sorted list of unique entity ids,
 * offsets non-decreasing) and q_grp [B], the group of each query (outside [0, n_grp): none); filt_rank[b] = rank[b] minus the members
 * other than the true id with d <= d_true.  grp_off == NULL: no filter, filt_rank = rank.  A query whose h, t or r lies outside its
 * table gets rank = filt_rank = 0 and reads nothing.  scores != NULL: also scores[b * n_ent + c] = -d, the values the ranks compare
 * (fp32 [B, n_ent]).  D % 4 == 0.  workspace >= ia_kgpt_lp_workspace_bytes(B, D) = O(B D), independent of n_ent. */
#define IA_KGPT_LP_TAIL 0
#define IA_KGPT_LP_HEAD 1
size_t ia_kgpt_lp_workspace_bytes(int B, int D);
int ia_kgpt_lp_rank(const float* ent, const float* rel, const int64_t* h, const int64_t* t, const int64_t* r, int B, int D, int n_ent,
                    int n_rel, int norm, int side, const int64_t* grp_off, const int64_t* grp_ids, int n_grp, const int64_t* q_grp,
                    int64_t* rank, int64_t* filt_rank, float* scores, void* workspace, size_t workspace_bytes, ia_stream_t stream);
/* Knowledge-graph completion (torchkge EntityInference / RelationInference): the k best candidates of each of B queries over the raw
 * tables (no normalisation, no projection term), without a [B, n_cand] matrix.  IA_KGPT_TOPK_TAILS: a = head ids, b = relation ids,
 * q = ent[a] + rel[b], candidates = the n_ent entity rows; IA_KGPT_TOPK_HEADS: a = tail ids, b = relation ids, q = ent[a] - rel[b],
 * candidates = entity rows; IA_KGPT_TOPK_RELS: a = head ids, b = tail ids, q = ent[b] - ent[a], candidates = the n_rel relation rows.
 * score_c = -d(q, cand_c), d as in ia_kgpt_lp_rank (one fp32 accumulator per pair summed in k order): in the entity modes the scores
 * are bit-identical to what ia_kgpt_lp_rank(..., scores) stores for the same pair.  idx (int64 [B, k]) / score (fp32 [B, k]): row b
 * holds the k best candidates of query b in the total order (score descending, id ascending); the result is a function of the tables,
 * the query and the filter alone (not of B, the query's place in the batch, the split count or the launch order).  Filter: the layout
 * of ia_kgpt_lp_rank (grp_off / grp_ids int64 CSR, each group a sorted list of unique candidate ids, q_grp[b] outside [0, n_grp): no
 * filter for that query; grp_off == NULL: no filter); the members of the query's group are never returned.  Unused trailing slots
 * (fewer than k candidates left, k > n_cand) hold idx = -1, score = -inf, and so does the whole row of a query whose a or b lies
 * outside its table (it reads nothing).  1 <= k <= IA_KGPT_TOPK_MAX_K, D % 4 == 0, norm 1 or 2.  max_splits caps the number of
 * candidate ranges the scan is split into (0: as the rank scan chooses); the result does not depend on it.  workspace >=
 * ia_kgpt_topk_workspace_bytes(B, D, n_cand, k, max_splits) = O(B D + B splits k), independent of n_cand. */
#define IA_KGPT_TOPK_TAILS 0
#define IA_KGPT_TOPK_HEADS 1
#define IA_KGPT_TOPK_RELS 2
#define IA_KGPT_TOPK_MAX_K 64
size_t ia_kgpt_topk_workspace_bytes(int B, int D, int n_cand, int k, int max_splits);
int ia_kgpt_topk(const float* ent, const float* rel, const int64_t* a, const int64_t* b, int B, int D, int n_ent, int n_rel, int norm,
                 int mode, const int64_t* grp_off, const int64_t* grp_ids, int n_grp, const int64_t* q_grp, int k, int max_splits,
                 int64_t* idx, float* score, void* workspace, size_t workspace_bytes, ia_stream_t stream);
/* Same-item retrieval: the k most similar catalogue rows of each of B query rows by inner product (cosine on normalised rows), on the
 * bf16 matrix cores, without a [B, n_cand] matrix.  (Added without an ABI bump: nothing existing changed its meaning.)
 * Prepared rows are bf16 [rows, pitch], pitch = ia_sim_row_pitch(D) elements = D rounded up to the scan's k-step (>= D; 0 for D < 1),
 * the columns D .. pitch - 1 zero, the buffer 16-byte aligned.  ia_sim_rows_bf16 makes them, one row per wave:
 * out[r][c] = bf16(x[r * ldx + c] * inv_r), inv_r = 1 (normalize 0: a plain round-to-nearest-even conversion) or
 * 1 / max(sqrt(sum_c x[r][c]^2), 1e-12) in fp32 (normalize 1; an all-zero row stays zero); nothing past column D of a row of x is read
 * (ldx >= D).  1 <= D <= 2^20.
 * ia_sim_topk: s[b][c] = sum_k q[b][k] cand[c][k] with one fp32 MFMA accumulator per pair that walks k in the same order whatever the
 * split count (splits are over candidates, never over k): the score of a pair is a function of the two rows alone.  idx (int64 [B, k]) /
 * score (fp32 [B, k]): row b holds the k best candidates of query b in the total order (score descending, candidate index ascending);
 * the result does not depend on B, the query's place in the batch, max_splits or the launch order.  Candidate skip[b] is never returned
 * to query b (-1, or any value outside [0, n_cand): skip none; skip == NULL: no query skips) -- how an item is kept out of its own
 * neighbour list.  Unused trailing slots (k > n_cand, or the only candidates skipped) hold idx = -1, score = -inf.  The inputs must
 * be finite (a NaN score has no place in the order).  1 <= k <= IA_SIM_TOPK_MAX_K; max_splits caps the number of candidate ranges
 * (0: the scan's choice).  B == 0 and n_cand == 0 are no errors (every slot unused).  Null q / cand / idx / score, k or D out of range,
 * negative sizes, misaligned rows and a workspace below ia_sim_topk_workspace_bytes(B, D, n_cand, k, max_splits) = O(B splits k)
 * (0 when B or n_cand is 0; NULL is accepted then) return IA_ERR_ARG before any launch. */
#define IA_SIM_TOPK_MAX_K 64
size_t ia_sim_row_pitch(int D);
int ia_sim_rows_bf16(const float* x, int ldx, int rows, int D, int normalize, void* out, ia_stream_t stream);
size_t ia_sim_topk_workspace_bytes(int B, int D, int n_cand, int k, int max_splits);
int ia_sim_topk(const void* q, const void* cand, int B, int D, int n_cand, const int64_t* skip, int k, int max_splits, int64_t* idx,
                float* score, void* workspace, size_t workspace_bytes, ia_stream_t stream);
/* The same scan over G ragged problems in one call: the hot path of an inverted-file index.  (Added without an ABI bump.)
 * Group g pairs the query rows [q_off[g], q_off[g + 1]) of q (prepared bf16 [P, pitch]) with the candidate rows
 * [c_off[g], c_off[g + 1]) of cand (prepared bf16 [n_cand, pitch]).  q_off and c_off are int64 [G + 1] arrays ON THE DEVICE,
 * non-decreasing, within [0, P] and [0, n_cand]; they are never read on the host, so the call launches and returns without a
 * synchronisation, and an offset out of range or out of order cannot be refused: it is clamped, or makes an empty range, inside the
 * kernels (no row outside the two matrices is touched; what such a group's rows receive is unspecified).  The grid is the upper bound
 * P / QT + G query tiles (QT = 256 rows for k <= 32, 128 above) and a workgroup finds its group by search.
 * idx (int64 [P, k]) / score (fp32 [P, k]): row p, a query row of group g, holds the k best candidates of group g in the total order
 * (score descending, REPORTED id ascending).  The reported id of candidate row c is label[c] (label_bits 32: int32, 64: int64; values in
 * [0, 2^31)), or c itself where label == NULL (label_bits 0).  The score of a pair is bit for bit what ia_sim_topk gives for the same
 * two rows; the result does not depend on the order of the groups, on how many share a call, on max_splits (the cap on the candidate
 * ranges a group is cut into; 0: the scan's choice; never over k) or on the launch order.  skip[p] is a POSITION in cand (not a
 * label): candidate row skip[p] is never returned to query row p; -1 or any row outside the group's range skips nothing; skip == NULL:
 * no row skips.  Groups without query rows, without candidates or with fewer than k candidates, and G == 0 or P == 0, are no errors:
 * unused trailing slots hold idx = -1, score = -inf.  Rows of q outside [q_off[0], q_off[G]) and rows of cand outside
 * [c_off[0], c_off[G]) are not read, and the rows of idx / score outside [q_off[0], q_off[G]) are not written.  A tail tile reads no row of
 * the next group.  Null q / cand / q_off / c_off / idx / score, a label without label_bits 32 or 64 (or label_bits without a label),
 * k or D out of range as for ia_sim_topk, negative sizes, q / cand / workspace off 16 bytes, another array off its element size, and a
 * workspace below ia_sim_topk_groups_workspace_bytes(P, G, D, n_cand, k, max_splits) (0 when P or G is 0) return IA_ERR_ARG before
 * any launch.
 * ia_sim_topk_fold: out row b = the k best, in the same total order, of the union of the rows rows_of[b * nprobe + j], j < nprobe, of
 * idx_in / score_in ([n_rows, k], as ia_sim_topk_groups writes them; rows_of: int64 on the device; -1 or a value outside [0, n_rows):
 * no list).  The lists of one b must hold no id twice (the lists of an index partition the catalogue and a query's probes are
 * distinct).  B == 0 is no error.
 * ia_sim_centroid_sums (k-means): sums[l][c] = the fp32 sum over i in [list_off[l], list_off[l + 1]), in that order, of
 * rows[order[i]][c] (rows: prepared bf16 [n_rows, pitch]; order: int64 [n_order], list_off: int64 [nlist + 1], both on the device;
 * sums: fp32 [nlist, D]; counts: int64 [nlist], the rows added).  One thread owns an output and adds in order, no atomics: equal inputs
 * give equal bits.  An empty list gives zeros and count 0; an order entry outside [0, n_rows) is left out. */
size_t ia_sim_topk_groups_workspace_bytes(int P, int G, int D, int n_cand, int k, int max_splits);
int ia_sim_topk_groups(const void* q, const void* cand, const int64_t* q_off, const int64_t* c_off, int G, int P, int D, int n_cand,
                       const void* label, int label_bits, const int64_t* skip, int k, int max_splits, int64_t* idx, float* score,
                       void* workspace, size_t workspace_bytes, ia_stream_t stream);
int ia_sim_topk_fold(const int64_t* idx_in, const float* score_in, int n_rows, const int64_t* rows_of, int B, int nprobe, int k,
                     int64_t* idx, float* score, ia_stream_t stream);
int ia_sim_centroid_sums(const void* rows, int n_rows, int D, const int64_t* order, int n_order, const int64_t* list_off, int nlist,
                         float* sums, int64_t* counts, ia_stream_t stream);

/* ---- whole-layer drivers: one call = every launch of one encoder layer, in order, on `stream`.
 * Weights: bf16 shadows for the GEMM operands, fp32 masters for bias / LayerNorm vectors. */
typedef struct {
  const void* w_qkv;   /* bf16 [3H, H]  query | key | value stacked (state_dict attention.self.{query,key,value}.weight) */
  const float* b_qkv;  /* fp32 [3H] */
  const void* w_o;     /* bf16 [H, H]   attention.output.dense.weight / timm attn.proj */
  const float* b_o;
  const float* ln1_g;  /* attention.output.LayerNorm (BERT post-LN) / norm1 (ViT pre-LN) */
  const float* ln1_b;
  const void* w_fc1;   /* bf16 [I, H]   intermediate.dense / mlp.fc1 */
  const float* b_fc1;
  const void* w_fc2;   /* bf16 [H, I]   output.dense / mlp.fc2 */
  const float* b_fc2;
  const float* ln2_g;  /* output.LayerNorm / norm2 */
  const float* ln2_b;
  /* (ABI 7) optional transposed bf16 copies, [H, 3H] / [H, H] / [H, I] / [I, H] (ia_transpose_bf16_batched keeps them in step with the
   * shadows above): the backward's data-gradient GEMMs dx = dy W then read W^T k-contiguously -- 2-16 % faster per launch than the
   * k-strided form (transpose reads out of LDS), 5.7 ms of a 434 ms step.  NULL = not provided (k-strided form). */
  const void* wt_qkv;
  const void* wt_o;
  const void* wt_fc1;
  const void* wt_fc2;
} ia_layer_weights;

typedef struct { /* fp32 gradient arena slots, same shapes as above; all accumulate (+=) */
  float* w_qkv; float* b_qkv; float* w_o; float* b_o; float* ln1_g; float* ln1_b;
  float* w_fc1; float* b_fc1; float* w_fc2; float* b_fc2; float* ln2_g; float* ln2_b;
} ia_layer_grads;

/* The lists of ONE row mask over B * L rows, each from its public builder (sizes: ia_row_*_bytes, ia_kblock_mask_bytes).  Device
 * pointers; each stands alone -- nothing is assumed about where one list sits relative to another -- and each is optional: NULL = the
 * layer call builds its own in its stash / scratch (one small launch).  A member the call's plan does not ask for is not read (which
 * plan reads which: ia_layer_cfg::key_rows / out_rows). */
typedef struct {
  const int* blocks;        /* ia_row_blocks */
  const int* packed;        /* ia_row_groups_packed */
  const int* slabs;         /* ia_row_slabs */
  const int* groups;        /* ia_row_groups */
  const uint32_t* kblocks;  /* ia_kblock_mask (32-row blocks of k) */
} ia_row_lists;
/* the bits of ia_layer_cfg::masked_rows_dead */
#define IA_ROWS_DEAD_BWD 1
#define IA_ROWS_DEAD_FWD 2

typedef struct {
  int B, L, H, I, nh;      /* tokens M = B*L; head dim = H/nh = 64 */
  int pre_ln;              /* 0 = BERT post-LN layer (RobertaLayer), 1 = ViT pre-LN block (timm Block) */
  float eps;               /* 1e-12 BERT / 1e-6 ViT */
  float hidden_drop, attn_drop;
  uint32_t seed;           /* per-step seed; the layer index is mixed in through layer_id */
  uint32_t layer_id;
  /* unpadded ("packed") sequences: when cu_seqlens (int32 [B+1], device) is not NULL the layer runs on total_tokens =
   * cu_seqlens[B] rows, sequence b owning rows cu_seqlens[b] .. cu_seqlens[b+1]; L is then the longest sequence and the
   * key_mask argument is ignored (every token of a sequence is attendable).  NULL / 0: padded [B, L] rows. */
  const int* cu_seqlens;
  int total_tokens;
  /* The query-row limit of a layer with out_row_live: 0 = off; n > 0 = the caller guarantees that out_row_live is zero at every position
   * >= n of every sequence, so the attention output there is unread and its gradient exactly zero.  The attention forward then computes
   * the query tiles that reach in front of n only (the other rows of the stash's context are zeros, written by the kernel) and the
   * attention backward treats the 32-query blocks at or beyond n as dead (ia_attn_fwd_q_rows / ia_attn_bwd_bias_q_rows); every output
   * row the caller reads and every gradient is bit-identical to out_q_rows = 0.  Honoured only together with out_row_live and on padded
   * rows (cu_seqlens == NULL). */
  int out_q_rows;
  /* pre-LN (ViT) stacks, backward only (ABI 5): the b_fc2 gradient of a block is the column sum of its incoming gradient dy, i.e. of
   * the input gradient dx the block ABOVE has just produced.  dx_colsum_out != NULL: this block's last LayerNorm backward also adds
   * the column sums of its dx into that fp32 [H] vector (pass the b_fc2 gradient slot of the block below); dy_colsum_done != 0: the
   * block above did that for this block's dy, so the separate column-sum pass over dy is skipped.  Zero / NULL = round-3 behaviour. */
  float* dx_colsum_out;
  int dy_colsum_done;
  /* Two promises of the caller about the masked positions (key_mask == 0); padded rows with a key mask only.  Any other bit: IA_ERR_ARG
   * from the layer calls, 0 from the three size functions.
   * IA_ROWS_DEAD_BWD: no output of a masked position reaches the loss, so the gradient arriving at such rows is exactly zero in every
   * layer.  The backward skips them: the attention backward the query blocks made of masked positions (IA_ATTN_MASKED_ROWS_DEAD), the
   * LayerNorm backwards the masked rows, the weight gradients the 32-row blocks of k without a live row, the data gradients the 8-row
   * slabs (x gelu' + column sums: the 32-row blocks packed by whole 128-row groups) without one; their rows of dx are zeros.
   * IA_ROWS_DEAD_FWD, only together with IA_ROWS_DEAD_BWD: nobody reads the layer's output at a masked position either, so the forward
   * of a post-LN layer skips too -- the GEMMs the 8-row slabs (the forward-only GELU: the 32-row blocks) made of masked positions, the
   * two LayerNorms the masked rows.  y, the LayerNorm outputs and sums are zeros at masked positions; q / k / v and the FFN activation
   * (with its derivative) are zeros in slabs without a live row; the two projection outputs are not written there (their LayerNorm
   * writes zeros over the stash's copy).  A stash written under both must be consumed by a backward with IA_ROWS_DEAD_BWD set.
   * Every value the unmasked positions produce, and every parameter gradient, is bit-identical to masked_rows_dead = 0. */
  int masked_rows_dead;
  /* The lists of key_mask taken as row_live [B * L] (ia_row_lists).  The mask is the same for every layer of a stack, forward and
   * backward: a caller builds them once per step and hands them to every call.  Read only under masked_rows_dead (padded rows,
   * post-LN):   forward (both promises): blocks, slabs;   backward: kblocks, packed (B * L <= 128 * 4096), slabs;   groups: not read. */
  ia_row_lists key_rows;
  /* Optional: a second live-row description for the part of the layer BEHIND the attention, a byte per row [B * L] (device).
   * Non-NULL = the caller guarantees that it reads this layer's output only in rows with out_row_live != 0 and that the gradient it hands
   * to the backward (dy, dy2) is all zeros in every other row; every such row must also be a live key.  The out-projection, the
   * LayerNorm behind it, fc1 + GELU, fc2 and (post-LN) the closing LayerNorm then run these rows only -- GEMMs by 32-row blocks -- and so
   * do their backward kernels; the x gelu' data gradient runs whole 128-row groups (ia_row_groups), which keeps the fc1 bias gradient
   * bit-identical.  The QKV projection, the attention, their backward and the pre-LN LN1 keep the key-mask filter (post-LN) or every row
   * (pre-LN): every row is a key (out_q_rows above limits the attention's QUERY rows).  y is unspecified outside out_row_live in a
   * pre-LN layer and zeros there in a post-LN layer; dx and every parameter gradient are bit-identical to the call without it.  Padded
   * rows only (cu_seqlens == NULL).  A stash written with out_row_live must be consumed by a backward with the same out_row_live. */
  const uint8_t* out_row_live;
  /* The lists of out_row_live.  A mask that depends on (B, L) only -- row 0 of each sequence -- is built once and kept.
   *   forward: blocks;   backward: kblocks, blocks, groups;   packed, slabs: not read. */
  ia_row_lists out_rows;
} ia_layer_cfg;

/* per-layer activation stash (saved by forward, read by backward) and shared backward scratch */
size_t ia_layer_stash_bytes(const ia_layer_cfg* cfg);
size_t ia_layer_bwd_scratch_bytes(const ia_layer_cfg* cfg);
/* x [M,H] bf16 -> y [M,H] bf16.  key_mask [B,L] uint8 or NULL.  stash (ia_layer_stash_bytes) receives what ia_layer_bwd needs. */
int ia_layer_fwd(const ia_layer_cfg* cfg, const ia_layer_weights* w, const void* x, const uint8_t* key_mask, void* y, void* stash,
                 ia_stream_t stream);
/* Forward only (evaluation / prediction; reference finetune_multimodal.py:470-563, 661-775 run the model under no_grad): the layer
 * without anything kept for a backward pass -- no gelu' stream, no pre-LayerNorm sums, dropout off whatever cfg says.  `scratch`
 * (>= ia_layer_infer_scratch_bytes) is transient: every layer of a stack may be handed the same buffer.  (ABI 5) */
size_t ia_layer_infer_scratch_bytes(const ia_layer_cfg* cfg);
int ia_layer_fwd_infer(const ia_layer_cfg* cfg, const ia_layer_weights* w, const void* x, const uint8_t* key_mask, void* y, void* scratch,
                       size_t scratch_bytes, ia_stream_t stream);
/* dy [M,H] bf16 -> dx [M,H] bf16 (dx may alias dy); parameter gradients accumulate into g. */
int ia_layer_bwd(const ia_layer_cfg* cfg, const ia_layer_weights* w, const ia_layer_grads* g, const void* x, const uint8_t* key_mask,
                 const void* y, const void* stash, const void* dy, void* dx, void* scratch, size_t scratch_bytes, ia_stream_t stream);
/* Split-residual form for stacks of post-LN layers: the gradient of the layer OUTPUT arrives as dy + dy2 (dy2 may be NULL) and the
 * gradient of the layer INPUT leaves as dx + dx2, dx2 being the residual-path part (the attention sub-block's LayerNorm input
 * gradient) - the next layer down takes (dx, dx2) as its (dy, dy2) and sums them inside its first LayerNorm backward, so no GEMM
 * carries a "+ aux" epilogue.  dx may alias dy, dx2 may alias dy2.  dx2 == NULL: dx holds the whole input gradient (bottom layer).
 * Pre-LN (ViT) layers: dy2 / dx2 must be NULL. */
int ia_layer_bwd2(const ia_layer_cfg* cfg, const ia_layer_weights* w, const ia_layer_grads* g, const void* x, const uint8_t* key_mask,
                  const void* y, const void* stash, const void* dy, const void* dy2, void* dx, void* dx2, void* scratch,
                  size_t scratch_bytes, ia_stream_t stream);

/* ---- GCNII graph encoder of the graph two-tower model (reference src/models/graph.py; csrc/gcn.hip), fp32 in and out.  (ABI 14)
 * The adjacency is CSR: rowptr int64 [N+1], col int32 or int64 [nnz] (col_is_64), val fp32 [nnz] or NULL = all ones.  C (node
 * width): a multiple of 32 in [32, 512]; N * max(C, F) < 2^32.  Matrices are row-major, 16-byte aligned.  A dropout mask is a
 * function of (seed, stream_id, element index): element e of stream s is kept iff the 16-bit half (e & 1) of ia_rng(seed, s, e >> 1)
 * is >= round(p * 65536); kept elements are scaled by 1 / (1 - round(p * 65536) / 65536).  No float atomics anywhere: results are
 * bit-identical from run to run.  long_rows (int32 [n_long]): the rows with more than IA_GCN_LONG_ROW neighbours; each is summed by a
 * whole workgroup instead of one wave.  The list must hold EVERY such row, or be NULL: with NULL every row is summed by one wave
 * (correct, slow for hub rows); with a list, a row over the limit that the list lacks is written by nobody.  A listed row at or
 * under the limit is left to its wave. */
#define IA_GCN_LONG_ROW 512
#define IA_GCN_SLAB_ROWS 1024   /* node rows per partial product of the weight gradients (the longest fp32 sum feeding dW) */
/* h = (1 - alpha) * A (drop(x)) + alpha * x0 */
int ia_gcn_propagate_fwd(const int64_t* rowptr, const void* col, int col_is_64, const float* val, const float* x, const float* x0,
                         float* h, int N, int C, float alpha, float drop_p, uint32_t seed, uint32_t stream_id,
                         const int32_t* long_rows, int n_long, ia_stream_t stream);
/* The same gather over the CSR of A^T: dx = keep / (1 - p) * (1 - alpha) * A^T dh  (overwritten; NULL: added into dx0 instead, for
 * the layer whose input x is x0 itself);  dx0 = (dx0_accumulate ? dx0 : 0) + alpha * dh. */
int ia_gcn_propagate_bwd(const int64_t* rowptr_t, const void* col_t, int col_is_64, const float* val_t, const float* dh, float* dx,
                         float* dx0, int dx0_accumulate, int N, int C, float alpha, float drop_p, uint32_t seed, uint32_t stream_id,
                         const int32_t* long_rows_t, int n_long_t, ia_stream_t stream);
/* out = drop(relu((1 - beta) h + beta h W)), W [C, C] (GCN2Conv weight1); drop_p = 0 for every layer but a last one whose output
 * dropout is fused here.  out > 0 exactly where the backward passes a gradient. */
int ia_gcn_mix_fwd(const float* h, const float* W, float* out, int N, int C, float beta, float drop_p, uint32_t seed, uint32_t stream_id,
                   ia_stream_t stream);
/* workspace of ia_gcn_mix_bwd (F = 0) and ia_gcn_input_bwd: ceil(N / IA_GCN_SLAB_ROWS) partial [C, max(C, F)] products */
size_t ia_gcn_workspace_bytes(int N, int C, int F);
/* dpre = dout * (out > 0) / (1 - p);  dh = (1 - beta) dpre + beta dpre W^T (overwritten, no aliasing);  dW += beta h^T dpre
 * (dW NULL: skipped). */
int ia_gcn_mix_bwd(const float* dout, const float* out, const float* h, const float* W, float* dh, float* dW, int N, int C, float beta,
                   float drop_p, void* workspace, size_t workspace_bytes, ia_stream_t stream);
/* x0 = relu(drop(X) W^T + bias): X [N, F] (F a multiple of 4), W [C, F], bias [C] */
int ia_gcn_input_fwd(const float* X, const float* W, const float* bias, float* x0, int N, int F, int C, float drop_p, uint32_t seed,
                     uint32_t stream_id, ia_stream_t stream);
/* dpre = dx0 * (x0 > 0);  dW += dpre^T drop(X);  db += column sums of dpre */
int ia_gcn_input_bwd(const float* dx0, const float* x0, const float* X, float* dW, float* db, int N, int F, int C, float drop_p,
                     uint32_t seed, uint32_t stream_id, void* workspace, size_t workspace_bytes, ia_stream_t stream);
/* out[r] = drop(x[idx[r]]), r < R (mask element r * C + c);  idx outside [0, N) reads a zero row */
int ia_gcn_pair_gather_fwd(const float* x, const int32_t* idx, float* out, int R, int C, int N, float drop_p, uint32_t seed,
                           uint32_t stream_id, ia_stream_t stream);
/* dnode[idx[r]] += drop-mask(r) * dout[r]; order int32 [R] = the rows r stably sorted by idx[r]: a node that occurs in several rows is
 * summed in that order by a single writer. */
int ia_gcn_pair_scatter_bwd(const float* dout, const int32_t* idx, const int32_t* order, float* dnode, int R, int C, int N, float drop_p,
                            uint32_t seed, uint32_t stream_id, ia_stream_t stream);

/* ---- TextCNN tower (reference src/models/text.py:1496-1527; csrc/textcnn.hip).  (ABI 15)
 * S filter sizes K_s (sizes: HOST array of S ints, S <= IA_TEXTCNN_MAX_SIZES), F filters each, NF = S * F features, NT = F * sum K_s
 * taps, NTP = NT rounded up to a multiple of 8.  W / bias / dW / db are HOST arrays of S device pointers, one per filter size, in the
 * layout of the reference's Conv2d(2, F, (K_s, H)): weight fp32 [F, 2, K_s, H], bias fp32 [F].  x_c [B * L, H] bf16 is the embedding
 * LayerNorm output of channel c.  The convolution runs as two ia_gemm_bf16 calls, P [B * L, ldp] (fp32) = x_0 taps_0^T, then
 * += x_1 taps_1^T (accumulate), against the tap shadow taps [2][NTP, H] bf16 whose row -- the column of P --
 *     n(s, k, f) = F * (K_0 + .. + K_{s-1}) + k * F + f          (size index, then k, then f)
 * holds W_s[f, c, k, :]; rows NT .. NTP-1 are zero.  pre[b, s, f, t] = bias_s[f] + sum_{k < K_s} P[b * L + t + k][n(s, k, f)].
 * IA_ERR_ARG: L < max K_s (the reference's Conv2d raises there), H % 8 != 0, a non-positive count, a dropout rate outside [0, 1).
 * The two dropouts (TextCNN.dropout, rate p1, and the pair head's own, rate p2) are independent draws on feature element
 * e = b * NF + j, j = s * F + f, of streams stream_id1 / stream_id2: each keeps e iff the 16-bit half (e & 1) of its 32-bit draw at
 * counter e >> 1 is >= round(p * 65536); an element both keep is scaled by 1 / ((1 - p1')(1 - p2')), p' = round(p * 65536) / 65536.
 * A rate of 0 draws nothing.  The backward calls re-evaluate the masks from the same (seed, stream ids). */
#define IA_TEXTCNN_MAX_SIZES 8
/* fp32 conv weights -> taps (every element of [2][NTP, H] written); run after each optimiser step */
int ia_textcnn_pack_taps(const float* const* W, const int* sizes, int S, int F, int H, void* taps, ia_stream_t stream);
/* feat [B, NF] fp32 = dropouts(max_t relu(pre)), argmax [B, NF] int32 = the winning t, ties to the lowest t; a feature whose best
 * pre-activation is <= 0 is exactly 0 with argmax -1 (it sends no gradient).  ldp >= NT. */
int ia_textcnn_pool_fwd(const float* P, int ldp, const float* const* bias, const int* sizes, int S, int F, int B, int L, float p1,
                        float p2, uint32_t seed, uint32_t stream_id1, uint32_t stream_id2, float* feat, int32_t* argmax,
                        ia_stream_t stream);
/* g [B, NF] fp32 = dloss/dfeat; g' = g * keep-and-scale where argmax >= 0, else 0.
 * dW_s[f, c, k, :] = sum_b g'[b, j] x_c[b, argmax[b, j] + k, :], db_s[f] = sum_b g'[b, j] (db may be NULL): overwritten, b summed in
 * index order, no atomics. */
int ia_textcnn_pool_bwd_w(const float* g, const int32_t* argmax, const void* x0, const void* x1, const int* sizes, int S, int F, int B,
                          int L, int H, float p1, float p2, uint32_t seed, uint32_t stream_id1, uint32_t stream_id2, float* const* dW,
                          float* const* db, ia_stream_t stream);
/* dx [B * L, H] bf16, every row written: dx[b, argmax[b, j] + k, :] = sum over the (s, f, k) that land there, in that order, of
 * g'[b, j] W_s[f, 0, k, :], in fp32 with one bf16 rounding; rows no winning window covers are exactly zero.  Channel 0 only
 * (embedding2 of the reference is frozen). */
int ia_textcnn_pool_bwd_x(const float* g, const int32_t* argmax, const float* const* W, const int* sizes, int S, int F, int B, int L,
                          int H, float p1, float p2, uint32_t seed, uint32_t stream_id1, uint32_t stream_id2, void* dx,
                          ia_stream_t stream);

/* ---- cross-entropy over vocabulary logits: nn.CrossEntropyLoss(ignore_index=-1) of the masked-LM head (pytorch_transformers
 * BertForPreTraining; reference bert_pretrain.py:564-569).  logits [M, ld] fp32 (ld >= V, ld % 4 == 0; columns V .. ld-1 are never
 * read), labels [M] int64.  lse[r] = log sum_j exp(logits[r][j]) (row maximum subtracted first), loss_row[r] = lse[r] - logits[r][label],
 * loss[0] = sum loss_row / n_live, loss[1] = n_live.  A row with label < 0 is ignored: nothing of it is read, lse = loss_row = 0, it
 * is not counted.  A label >= V reads nothing out of bounds: that row's loss_row, hence the mean, is NaN.  n_live == 0: the mean is
 * NaN, as torch's.  Fixed summation order, no atomics: two runs are bit-identical.  IA_ERR_ARG / IA_ERR_WORKSPACE before any launch.
 * ia_vocab_ce_bwd: dlogits [M, ldg] bf16 (ldg >= V, ldg % 8 == 0) = bf16((exp(logits - lse) - onehot(label)) * dloss[0] / loss[1]) in
 * columns < V, exact zeros in columns V .. ldg-1 and in every row that is ignored or whose label is >= V: the A operand of the
 * hidden-gradient GEMM (k-contiguous) and of the table-gradient GEMM (k-strided) as it stands.  The additions did not
 * bump IA_ABI_VERSION: nothing existing changed its meaning. */
size_t ia_vocab_ce_workspace_bytes(int M);
int ia_vocab_ce_fwd(const float* logits, int ld, const int64_t* labels, float* lse, float* loss_row, float* loss /* [2]: mean, n_live */,
                    int M, int V, void* workspace, size_t workspace_bytes, ia_stream_t stream);
int ia_vocab_ce_bwd(const float* logits, int ld, const int64_t* labels, const float* lse, const float* loss /* reads [1] */,
                    const float* dloss /* device scalar */, void* dlogits /* bf16 [M, ldg] */, int ldg, int M, int V, ia_stream_t stream);

/* ---- symmetric contrastive loss between the text and the image embeddings of a batch (CoCaForPretraining; reference
 * src/models/multimodal.py:843-933).  text [B, ldt], image [B, ldi] fp32 (ld >= H), log_scale a device scalar, s = expf(*log_scale).
 * ia_contrastive_fwd: sim [B, lds] fp32 (lds >= B) = s text image^T in fp32 FMA, lse_row[i] = log sum_j exp(sim[i][j]), lse_col[j] =
 * log sum_i exp(sim[i][j]) (maximum subtracted first), loss[0] = 0.5 (mean_i (lse_row[i] - sim[i][i]) + mean_j (lse_col[j] -
 * sim[j][j])) = 0.5 (CE(sim, arange) + CE(sim^T, arange)).  sim, lse_row and lse_col are what the backward call reads.
 * ia_contrastive_bwd: G[i][j] = dloss[0] (0.5 / B) (exp(sim[i][j] - lse_row[i]) + exp(sim[i][j] - lse_col[j]) - 2 [i == j]);
 * dtext [B, lddt] = s G image, dimage [B, lddi] = s G^T text, dlog_scale[0] = (accumulate_dlog_scale ? dlog_scale[0] : 0) +
 * sum_ij G[i][j] sim[i][j].  Any B >= 1, H >= 1.  The pad columns of the inputs are never read, those of the outputs never written.
 * Fixed summation order, no atomics: two runs are bit-identical.  IA_ERR_ARG / IA_ERR_WORKSPACE before any launch; the workspace of
 * ia_contrastive_workspace_bytes(B) serves both calls and carries nothing from one to the other.  The additions did not
 * bump IA_ABI_VERSION: nothing existing changed its meaning. */
size_t ia_contrastive_workspace_bytes(int B);
int ia_contrastive_fwd(const float* text, int ldt, const float* image, int ldi, const float* log_scale /* device scalar */,
                       float* sim /* [B, lds] fp32, scaled; kept for backward */, int lds, float* lse_row, float* lse_col,
                       float* loss /* [1] */, int B, int H, void* workspace, size_t workspace_bytes, ia_stream_t stream);
int ia_contrastive_bwd(const float* text, int ldt, const float* image, int ldi, const float* log_scale, const float* sim, int lds,
                       const float* lse_row, const float* lse_col, const float* dloss /* device scalar */, float* dtext, int lddt,
                       float* dimage, int lddi, float* dlog_scale /* [1] */, int accumulate_dlog_scale, int B, int H, void* workspace,
                       size_t workspace_bytes, ia_stream_t stream);

/* ---- the same loss for one rank's shard of a global batch (data-parallel CoCa pre-training).  `world` ranks share a global batch of
 * G items; this rank holds its rows row_offset .. row_offset + B - 1 as text_l, image_l [B, ld >= H]; text_g, image_g [G, ld >= H] are
 * the embeddings of all ranks, gathered rank-major (the caller's collective).  den = (float)G / (float)world.
 * ia_contrastive_shard_fwd: sim_t [B, lds] (lds >= G) = s text_l image_g^T, rows row_offset + i of the global sim; sim_i [B, lds] =
 * s image_l text_g^T, its columns row_offset + i, transposed; lse_row_l[i], lse_col_l[i] their row log-sum-exps, i.e. the global
 * lse_row / lse_col at row_offset + i; loss[0] = 0.5 (sum_i (lse_row_l[i] - sim_t[i][row_offset + i]) / den + sum_i (lse_col_l[i] -
 * sim_i[i][row_offset + i]) / den).  The mean of the ranks' losses is ia_contrastive_fwd's loss of the global batch.
 * ia_contrastive_shard_bwd: lse_row_g, lse_col_g [G] are the lse_*_l of all ranks, gathered like the embeddings.  With c = dloss[0]
 * (0.5 / den) and d = row_offset + i: Gt[i][j] = c (exp(sim_t[i][j] - lse_row_g[d]) + exp(sim_t[i][j] - lse_col_g[j]) - 2 [j == d]),
 * Gi[i][j] = c (exp(sim_i[i][j] - lse_col_g[d]) + exp(sim_i[i][j] - lse_row_g[j]) - 2 [j == d]); dtext_l [B, lddt] = s Gt image_g,
 * dimage_l [B, lddi] = s Gi text_g, dlog_scale[0] = (accumulate_dlog_scale ? dlog_scale[0] : 0) + sum_ij Gt[i][j] sim_t[i][j].  These
 * are `world` times the rank's share of the global-batch gradient: averaged over the ranks (dlog_scale) or taken row by row (dtext_l,
 * dimage_l, divided by world) they are ia_contrastive_bwd's of the global batch, so the backward needs no collective and nothing
 * flows back through text_g / image_g.  B >= 1, 0 <= row_offset, row_offset + B <= G, world >= 1, H >= 1.  fp32 FMA, fixed summation
 * order, no atomics: two runs are bit-identical, and at world = 1, row_offset = 0, G = B every output is bit-identical to
 * ia_contrastive_fwd / ia_contrastive_bwd.  Pad columns are never read and never written.  IA_ERR_ARG / IA_ERR_WORKSPACE before any
 * launch; the workspace of ia_contrastive_shard_workspace_bytes(B, G) serves both calls and carries nothing from one to the other.
 * The additions did not bump IA_ABI_VERSION: nothing existing changed its meaning. */
size_t ia_contrastive_shard_workspace_bytes(int B, int G);
int ia_contrastive_shard_fwd(const float* text_l, int ldtl, const float* image_l, int ldil, const float* text_g, int ldtg,
                             const float* image_g, int ldig, const float* log_scale /* device scalar */, float* sim_t, float* sim_i,
                             int lds, float* lse_row_l, float* lse_col_l, float* loss /* [1] */, int B, int G, int row_offset, int world,
                             int H, void* workspace, size_t workspace_bytes, ia_stream_t stream);
int ia_contrastive_shard_bwd(const float* text_g, int ldtg, const float* image_g, int ldig, const float* log_scale, const float* sim_t,
                             const float* sim_i, int lds, const float* lse_row_g, const float* lse_col_g,
                             const float* dloss /* device scalar */, float* dtext_l, int lddt, float* dimage_l, int lddi,
                             float* dlog_scale /* [1] */, int accumulate_dlog_scale, int B, int G, int row_offset, int world, int H,
                             void* workspace, size_t workspace_bytes, ia_stream_t stream);

/* ---- data-parallel gradient exchange (pure data parallelism, one process per GPU; reference loop being sharded:
 * finetune_multimodal.py:371-468).  RCCL over xGMI behind four calls, for hosts that bind only this header (the Python host of this
 * repository uses torch.distributed, i.e. the same RCCL).  Rank 0 obtains an id and hands its IA_COMM_ID_BYTES bytes to the other
 * ranks by any out-of-band means; every rank then calls ia_comm_init (collective).  ia_comm_allreduce_bucket sums `count` elements in
 * place across the ranks, asynchronously on `stream` -- the caller launches it per gradient bucket as soon as the bucket's last
 * gradient kernel has been enqueued on that stream (or on a side stream ordered behind it) and divides by the world size in its
 * optimiser step (ia_adamw_flat's grad_scale).  RCCL is bound with dlopen at the first call (a copy already mapped into the process
 * is reused, whatever file name it was loaded under); IA_ERR_UNSUPPORTED = no librccl, a symbol missing, or not the 2.x API --
 * ia_comm_last_error() has the text (per calling thread).  PRECONDITION of ia_comm_init and ia_comm_allreduce_bucket: the calling
 * thread's current HIP device (hipSetDevice) is the GPU this rank owns -- RCCL binds the communicator to it.  (ABI 5) */
#define IA_COMM_ID_BYTES 128
#define IA_COMM_F32 0
#define IA_COMM_BF16 1
int ia_comm_unique_id(void* id_out);
int ia_comm_init(const void* id, int rank, int world_size, void** comm_out);
int ia_comm_allreduce_bucket(void* comm, void* buf, size_t count, int dtype, ia_stream_t stream);
int ia_comm_finalize(void* comm);
const char* ia_comm_last_error(void);

#ifdef __cplusplus
}
#endif
#endif /* ITEMALIGN_H */
