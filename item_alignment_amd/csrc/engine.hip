// Whole-layer drivers: every launch of one encoder layer (forward or backward) issued in order on
// the caller's HIP stream from native code, so the Python host pays one call per layer instead of
// one per op.  Two layer shapes share the same kernels:
//   post-LN  RoBERTa/BERT layer  (transformers RobertaLayer, called at reference src/models/text.py:1241,
//            src/models/multimodal.py:185, src/models/text.py:264)
//   pre-LN   ViT block           (timm vision_transformer.Block, called at src/models/multimodal.py:811,
//            src/models/image.py:459)
#include "common.h"
#include "../../include/itemalign.h"

namespace {

inline size_t al(size_t b) { return (b + 255) & ~(size_t)255; }
// token rows of the layer: B*L padded rows, or the packed total when the sequences are unpadded (cu_seqlens)
inline size_t rows_of(const ia_layer_cfg* c) { return c->cu_seqlens ? (size_t)c->total_tokens : (size_t)c->B * c->L; }

// hands out consecutive 256-byte-aligned pieces of one allocation (a null base only counts the bytes)
struct Carver {
  char* base; size_t bytes = 0;
  char* take(size_t b) { char* r = base ? base + bytes : nullptr; bytes += al(b); return r; }
};

// Where a layer call builds the row lists its caller did not hand in (resolve_rows): one slot per filter kind, null where the call
// never builds that kind
struct RowSlots { uint32_t* kmask = nullptr; int* blocks = nullptr; int* groups = nullptr; int* packed = nullptr; int* slabs = nullptr; uint32_t* ksteps = nullptr; };

// The buffers of one layer forward, by role.  The training stash gives each role its own memory (the backward reads them all); the
// forward-only scratch aliases the ones whose contents are dead by the time the memory is written again.
struct FwdBufs {
  char* qkv; char* ctx;
  char* xn;     // pre-LN only: LN1(x), the QKV projection's input
  char* proj;   // attention output projection; the LayerNorm after it leaves the residual sum here (post-LN: z1, pre-LN: x1)
  char* ln;     // the LayerNorm output that feeds the FFN (post-LN: y1 = LN1(z1), pre-LN: LN2(x1))
  char* ffn;    // post-LN only: FFN output, then z2 in place (pre-LN writes the layer output straight from the fc2 epilogue)
  char* hpre;   // gelu'(pre-activation) (IA_EPI_BIAS_GELU C2); null in the forward-only form
  char* hact;   // FFN hidden activation
  float* lse; float* mean1; float* rstd1; float* mean2; float* rstd2;
  RowSlots key;  // IA_ROWS_DEAD_FWD: the forward's own 32-row block list and 8-row slab list of the key mask
  RowSlots out;  // out_row_live: the forward's own block list of it
  size_t bytes;
};

// the three [M, H] row buffers in the order the layer shape uses them
void name_rows(FwdBufs& s, bool pre_ln, char* t0, char* t1, char* t2) {
  if (pre_ln) { s.xn = t0; s.proj = t1; s.ln = t2; s.ffn = nullptr; }
  else { s.xn = nullptr; s.proj = t0; s.ln = t1; s.ffn = t2; }
}

FwdBufs carve_stash(const ia_layer_cfg* c, void* base) {
  const size_t M = rows_of(c), H = c->H, I = c->I;
  Carver a{(char*)base};
  FwdBufs s;
  s.qkv = a.take(M * 3 * H * 2); s.ctx = a.take(M * H * 2);
  char* t0 = a.take(M * H * 2); char* t1 = a.take(M * H * 2); char* t2 = a.take(M * H * 2);
  name_rows(s, c->pre_ln, t0, t1, t2);
  s.hpre = a.take(M * I * 2); s.hact = a.take(M * I * 2);
  s.lse = (float*)a.take((size_t)c->B * c->nh * c->L * 4);
  s.mean1 = (float*)a.take(M * 4); s.rstd1 = (float*)a.take(M * 4);
  s.mean2 = (float*)a.take(M * 4); s.rstd2 = (float*)a.take(M * 4);
  s.key.blocks = (int*)a.take(ia_row_blocks_bytes((int)M));
  s.out.blocks = (int*)a.take(ia_row_blocks_bytes((int)M));
  s.key.slabs = (int*)a.take(ia_row_slabs_bytes((int)M));
  s.bytes = a.bytes;
  return s;
}

// forward only: no gelu' stream, one pair of LayerNorm statistics, and two row buffers -- the third role reuses t0 once its first
// contents are consumed (post-LN: z1 by LN1, pre-LN: LN1(x) by the QKV projection)
FwdBufs carve_infer(const ia_layer_cfg* c, void* base) {
  const size_t M = rows_of(c), H = c->H, I = c->I;
  Carver a{(char*)base};
  FwdBufs s;
  s.qkv = a.take(M * 3 * H * 2); s.ctx = a.take(M * H * 2);
  char* t0 = a.take(M * H * 2); char* t1 = a.take(M * H * 2);
  name_rows(s, c->pre_ln, t0, t1, t0);
  s.hpre = nullptr; s.hact = a.take(M * I * 2);
  s.lse = (float*)a.take((size_t)c->B * c->nh * c->L * 4);
  s.mean1 = s.mean2 = (float*)a.take(M * 4); s.rstd1 = s.rstd2 = (float*)a.take(M * 4);
  s.key.blocks = (int*)a.take(ia_row_blocks_bytes((int)M));
  s.out.blocks = (int*)a.take(ia_row_blocks_bytes((int)M));
  s.key.slabs = (int*)a.take(ia_row_slabs_bytes((int)M));
  s.bytes = a.bytes;
  return s;
}

struct Scratch {
  char* g0; char* g1; char* g2; char* gI; char* gqkv; float* delta; char* ws; size_t ws_bytes; char* gws; size_t gws_bytes;
  RowSlots key;      // masked_rows_dead: the key mask's 32-row block mask (ia_kblock_mask), block-packed list, 8-row slab list, step mask
  RowSlots out;      // out_row_live: its 32-row block mask, block list, group list and 16-row step mask (ia_kstep_mask)
  size_t bytes;
};

size_t max3(size_t a, size_t b, size_t c) { return a > b ? (a > c ? a : c) : (b > c ? b : c); }

Scratch carve_scratch(const ia_layer_cfg* c, void* base) {
  const size_t M = rows_of(c), H = c->H, I = c->I;
  Carver a{(char*)base};
  Scratch s;
  s.g0 = a.take(M * H * 2); s.g1 = a.take(M * H * 2); s.g2 = a.take(M * H * 2);
  s.gI = a.take(M * I * 2); s.gqkv = a.take(M * 3 * H * 2);
  s.delta = (float*)a.take((size_t)c->B * c->nh * c->L * 4);
  s.ws_bytes = max3(ia_ln_bwd_workspace_bytes((int)M, (int)H), ia_gemm_colsum_workspace_bytes((int)M, (int)I),
                    max3(ia_colsum_workspace_bytes((int)M, (int)(3 * H)), ia_attn_bwd_bias_workspace_bytes(c->B, c->nh, c->L), 0));
  s.ws = a.take(s.ws_bytes);
  // split-K partial sums of the four weight-gradient GEMMs (largest of them)
  s.gws_bytes = max3(ia_gemm_workspace_bytes((int)(3 * H), (int)H, (int)M, 1), ia_gemm_workspace_bytes((int)I, (int)H, (int)M, 1),
                     max3(ia_gemm_workspace_bytes((int)H, (int)I, (int)M, 1), ia_gemm_workspace_bytes((int)H, (int)H, (int)M, 1), 0));
  s.gws = a.take(s.gws_bytes);
  // masked_rows_dead: which 32-row blocks of the weight gradients' k hold a live row (one bit each, ia_kblock_mask)
  s.key.kmask = (uint32_t*)a.take(ia_kblock_mask_bytes((int)M));
  // ... and the data gradients' lists of them: the live blocks packed by whole groups, the 8-row slabs (below)
  s.key.packed = (int*)a.take(ia_row_groups_packed_bytes((int)M));
  s.out.kmask = (uint32_t*)a.take(ia_kblock_mask_bytes((int)M));
  s.out.blocks = (int*)a.take(ia_row_blocks_bytes((int)M));
  s.out.groups = (int*)a.take(ia_row_groups_bytes((int)M));
  s.key.slabs = (int*)a.take(ia_row_slabs_bytes((int)M));
  // the weight gradients' 16-row step masks (ia_kstep_mask), always built here: ia_row_lists has no member for them.  Behind everything
  // else: a reader of the scratch finds every other piece where it was.
  s.key.ksteps = (uint32_t*)a.take(ia_kstep_mask_bytes((int)M));
  s.out.ksteps = (uint32_t*)a.take(ia_kstep_mask_bytes((int)M));
  s.bytes = a.bytes;
  return s;
}

bool cfg_ok(const ia_layer_cfg* c) {
  if (c && c->cu_seqlens && (c->total_tokens <= 0 || c->total_tokens > c->B * c->L)) return false;
  if (c && (c->masked_rows_dead & ~(IA_ROWS_DEAD_BWD | IA_ROWS_DEAD_FWD))) return false;   // (an older caller's layout bits: refused)
  return c && c->B > 0 && c->L > 0 && c->H > 0 && c->I > 0 && c->nh > 0 && c->H == c->nh * 64 && (c->H & 7) == 0 && (c->I & 7) == 0;
}

// Diagnostics: 0 withholds their lists from the data gradients of ia_layer_bwd2 (they run every row); returns the previous setting.
int g_dgrad_rows = 1;
// ... and 0 makes layer_forward run every row under IA_ROWS_DEAD_FWD (ia_debug_fwd_rows)
int g_fwd_rows = 1;
// ... and 0 makes the layer calls ignore ia_layer_cfg::out_row_live (ia_debug_out_rows)
int g_out_rows = 1;
// out_row_live (ia_layer_cfg): the rows the caller reads of this layer's output, and the only rows whose incoming gradient is not zero.
// Everything behind the attention runs these rows only; in front of it every row is a key and stays.  Padded rows only.
const uint8_t* out_live(const ia_layer_cfg* c) { return (c->out_row_live && !c->cu_seqlens && g_out_rows) ? c->out_row_live : nullptr; }
// ... and 0 makes them ignore ia_layer_cfg::out_q_rows (ia_debug_q_rows)
int g_q_rows = 1;
// out_q_rows (ia_layer_cfg): out_row_live is zero at every position >= n of every sequence, so the attention output there is unread and
// its gradient exactly zero -- the attention forward and backward run the query blocks in front of n only.  Only together with out_row_live.
int out_q_rows(const ia_layer_cfg* c) { return (out_live(c) && c->out_q_rows > 0 && g_q_rows) ? c->out_q_rows : 0; }

#define IA_TRY(expr) do { int rc_ = (expr); if (rc_) return rc_; } while (0)

// The rows one stretch of a layer call runs: their live bytes (null: every row) and, per kind, the filter made from them (IaRowFilter,
// common.h).  A kind nobody asked for, and every kind of an every-row plan, stays NONE.
struct RowPlan {
  const uint8_t* live = nullptr;
  IaRowFilter kmask, blocks, groups, packed, slabs, ksteps;
};
enum RowSource { KEY_MASK, OUT_ROWS };
enum : unsigned { WANT_KMASK = 1, WANT_BLOCKS = 2, WANT_GROUPS = 4, WANT_PACKED = 8, WANT_SLABS = 16, WANT_KSTEPS = 32 };

// The one place that builds the lists a caller did not hand in.  `live`: the key mask (its filters exist under IA_ROWS_DEAD_BWD on padded
// rows only) or out_row_live; null: an every-row plan.  For each kind of `want` the plan takes the caller's member of ia_row_lists
// (key_rows / out_rows: the mask is the same for every layer of a stack and step, so a caller builds them once), else one built here
// into `slot` (one small launch).  The packed list serves M <= 128 * 4096 rows (ia_row_groups_packed); beyond, none.
int resolve_rows(const ia_layer_cfg* c, RowSource which, const uint8_t* live, unsigned want, int M, const RowSlots& slot, ia_stream_t st,
                 RowPlan* plan) {
  *plan = RowPlan{};
  const bool key = which == KEY_MASK;
  if (!live || (key && (!(c->masked_rows_dead & IA_ROWS_DEAD_BWD) || c->cu_seqlens))) return IA_OK;
  plan->live = live;
  const ia_row_lists& given = key ? c->key_rows : c->out_rows;
  auto take = [&](IaRowFilter& f, IaRowFilter::Kind kind, const void* theirs, void* own) {
    f = IaRowFilter{kind, theirs ? theirs : own};
    return theirs ? IA_OK : ia_row_filter_build(kind, live, M, own, st);
  };
  if (want & WANT_KMASK) IA_TRY(take(plan->kmask, IaRowFilter::KBLOCKS, given.kblocks, slot.kmask));
  if (want & WANT_BLOCKS) IA_TRY(take(plan->blocks, IaRowFilter::BLOCKS, given.blocks, slot.blocks));
  if (want & WANT_GROUPS) IA_TRY(take(plan->groups, IaRowFilter::GROUPS, given.groups, slot.groups));
  if ((want & WANT_PACKED) && (size_t)M <= (size_t)128 * 4096) IA_TRY(take(plan->packed, IaRowFilter::PACKED, given.packed, slot.packed));
  if (want & WANT_SLABS) IA_TRY(take(plan->slabs, IaRowFilter::SLABS, given.slabs, slot.slabs));
  if (want & WANT_KSTEPS) IA_TRY(take(plan->ksteps, IaRowFilter::KSTEPS, nullptr, slot.ksteps));      // (no member of ia_row_lists: always built here)
  return IA_OK;
}

// Data gradient dx[M, n_in] = dy[M, k_out] W[k_out, n_in] (+ epilogue): through the transposed shadow wt[n_in, k_out] when the caller
// provides one (both operands k-contiguous: the faster form, ia_layer_weights::wt_*), else W read k-strided.
// Over the live rows of the plan, the other rows of dx written as zeros: the 8-row slabs where the epilogue has a slab form, else the
// 32-row blocks.  IA_EPI_DGELU_COLSUM never takes the plain blocks -- that remap would regroup the column-sum partials, and the fc1 bias
// gradient would equal the unfiltered one only up to fp32 summation order -- but whole 128-row groups (every kept partial stays where
// and what it was) or else the blocks packed by whole groups (each group's partial is formed by one wave from that group's live blocks
// in order and stored in the group's slot): both bit-identical to the every-row call.  No list: every row.
int dgrad(const void* dy, int k_out, const void* w, const void* wt, int n_in, void* dx, int M, int epilogue, const void* aux, int ldaux, void* c2,
          void* ws, size_t ws_bytes, ia_stream_t st, const RowPlan& rows) {
  IaRowFilter f = rows.blocks;
  if (epilogue == IA_EPI_DGELU_COLSUM) f = rows.groups ? rows.groups : rows.packed;
  else if (rows.slabs && ia_gemm_dgrad_form(IaRowFilter::SLABS, epilogue)) f = rows.slabs;
  return ia_gemm_dgrad_filtered(dy, k_out, wt ? wt : w, wt ? 0 : 1, wt ? k_out : n_in, dx, n_in, M, n_in, k_out, epilogue, aux, ldaux, c2, f, ws,
                                ws_bytes, st);
}

// Weight gradient dW[n_out, n_in] += dy[M, n_out]^T x[M, n_in] over the live k of the plan: the 16-row steps that hold a live row (an
// ia_kstep_mask) where the shape takes that walk, else the 32-row blocks (an ia_kblock_mask); an every-row plan: every row
bool wgrad_steps(int n_out, int n_in, int M) { return ia_gemm_wgrad_walk(n_out, n_in, M) == 2; }
int wgrad(const void* dy, int n_out, const void* x, int n_in, float* dw, int M, const RowPlan& rows, void* ws, size_t ws_bytes, ia_stream_t st) {
  const IaRowFilter f = (rows.ksteps && wgrad_steps(n_out, n_in, M)) ? rows.ksteps : rows.kmask;
  return ia_gemm_wgrad_filtered(dy, n_out, x, n_in, dw, n_in, n_out, n_in, M, f, 1, ws, ws_bytes, st);
}
// the masks a backward asks for: the step mask when one of the shapes it serves walks steps, the block mask when one does not
unsigned want_wgrad_masks(const int (*shapes)[2], int n, int M) {
  unsigned want = 0;
  for (int i = 0; i < n; ++i) want |= wgrad_steps(shapes[i][0], shapes[i][1], M) ? WANT_KSTEPS : WANT_KMASK;
  return want;
}

// A forward GEMM y[M, N] = x[M, K] w[N, K]^T (+ epilogue; aux has y's pitch) over the live rows of the plan: the 8-row slabs where the
// epilogue has a slab form (a sequence's rows never line up with 32-row blocks), else the 32-row blocks; no list: every row.
// fill: the dead rows of y (and c2) are written as zeros -- somebody reads every row -- else they are not written at all.
int fwd_gemm(const void* x, int K, const void* w, void* y, int N, int M, int epilogue, const float* bias, const void* aux, void* c2,
             const RowPlan& rows, bool fill, ia_stream_t st) {
  IaRowFilter f = (rows.slabs && ia_gemm_fwd_form(IaRowFilter::SLABS, epilogue)) ? rows.slabs : rows.blocks;
  f.fill = fill;
  return ia_gemm_fwd_filtered(x, K, w, K, y, N, M, N, K, epilogue, bias, aux, aux ? N : 0, c2, 0, 1.f, f, st);
}

// The QKV projection of a layer writes q already multiplied by softmax scale * log2(e) (one bf16 rounding, in the GEMM epilogue where
// the value is still fp32) and the attention kernels are told so: none of forward / dQ / dK-dV / fused backward re-scales its q tiles.
// Needs the q | k boundary on a 128-column tile boundary of the GEMM; other hidden sizes take the plain projection and kernels.
// With a filter (the key mask's slabs), the live rows only and the others as zeros: the attention kernels read every row of q, k and v.
bool q_prescale(const ia_layer_cfg* c) { return (c->H & 127) == 0; }
int qkv_proj(const ia_layer_cfg* c, const void* x, const ia_layer_weights* w, void* qkv, int M, float scale, ia_stream_t st, IaRowFilter rows) {
  const int H = c->H;
  const bool ps = q_prescale(c);
  return ia_gemm_fwd_filtered(x, H, w->w_qkv, H, qkv, 3 * H, M, 3 * H, H, IA_EPI_BIAS, w->b_qkv, nullptr, 0, nullptr, ps ? H : 0,
                              ps ? scale * 1.4426950408889634f : 1.f, rows, st);
}

// self-attention over the packed qkv projection [rows, 3H]: padded [B, L] rows with a key mask, or packed rows (cu_seqlens)
int attn_fwd(const ia_layer_cfg* c, const char* qkv, const uint8_t* key_mask, char* ctx, float* lse, float scale, float drop, uint32_t seed,
             ia_stream_t st) {
  const int H = c->H;
  const bool ps = q_prescale(c);
  if (c->cu_seqlens)
    return (ps ? ia_attn_fwd_varlen_ps : ia_attn_fwd_varlen)(qkv, qkv + (size_t)H * 2, qkv + (size_t)2 * H * 2, 3 * H, c->cu_seqlens, c->total_tokens, ctx, H, lse, c->B, c->nh,
                              c->L, scale, drop, seed, st);
  // (the rows the limit skips leave the kernel as zeros: the stash's ctx is finite in every row, whatever the buffer held)
  return ia_attn_fwd_q_rows(ps ? IA_ATTN_Q_PRESCALED : 0, qkv, qkv + (size_t)H * 2, qkv + (size_t)2 * H * 2, 3 * H, key_mask, ctx, H, lse, c->B, c->nh,
                            c->L, scale, drop, seed, out_q_rows(c), st);
}

// attention backward + the QKV bias gradient (+= into db_qkv): padded rows take the column sums out of the attention kernels'
// epilogues, packed rows (cu_seqlens) keep the separate column-sum pass over [rows, 3H]
int attn_bwd(const ia_layer_cfg* c, const char* qkv, const uint8_t* key_mask, const char* ctx, const char* dctx, const float* lse, float* delta,
             char* gqkv, float* db_qkv, void* ws, size_t ws_bytes, float scale, float drop, uint32_t seed, ia_stream_t st) {
  const int H = c->H;
  const bool ps = q_prescale(c);
  if (c->cu_seqlens) {
    int rc = (ps ? ia_attn_bwd_varlen_ps : ia_attn_bwd_varlen)(qkv, qkv + (size_t)H * 2, qkv + (size_t)2 * H * 2, 3 * H, c->cu_seqlens, c->total_tokens, ctx, dctx, H, lse, delta,
                                gqkv, gqkv + (size_t)H * 2, gqkv + (size_t)2 * H * 2, 3 * H, c->B, c->nh, c->L, scale, drop, seed, st);
    return rc ? rc : ia_colsum(gqkv, 3 * H, (int)rows_of(c), 3 * H, db_qkv, 1, ws, ws_bytes, st);
  }
  const int flags = (ps ? IA_ATTN_Q_PRESCALED : 0) | ((c->masked_rows_dead & IA_ROWS_DEAD_BWD) ? IA_ATTN_MASKED_ROWS_DEAD : 0);
  return ia_attn_bwd_bias_q_rows(flags, qkv, qkv + (size_t)H * 2, qkv + (size_t)2 * H * 2, 3 * H, key_mask, ctx, dctx, H, lse, delta, gqkv,
                                 gqkv + (size_t)H * 2, gqkv + (size_t)2 * H * 2, 3 * H, db_qkv, ws, ws_bytes, c->B, c->nh, c->L, scale, drop, seed,
                                 out_q_rows(c), st);
}

// Every launch of one layer forward.  keep = the training form, which leaves what the backward needs in s: the dropout masks' seeds,
// gelu'(pre-activation) beside the activation, and the post-LN residual sums z1 / z2.  Without it (evaluation / prediction, reference
// finetune_multimodal.py:470-563, 661-775) the launches and roundings are the same -- evaluation reproduces the training forward bit for
// bit when dropout is off -- minus those outputs, so s may alias buffers (carve_infer).
int layer_forward(const ia_layer_cfg* c, const ia_layer_weights* w, const void* x, const uint8_t* key_mask, void* y, const FwdBufs& s,
                  bool keep, ia_stream_t st) {
  const int M = (int)rows_of(c), H = c->H, I = c->I;
  const float scale = 0.125f;  // 1/sqrt(64)
  const int gelu = keep ? IA_EPI_BIAS_GELU : IA_EPI_BIAS_GELU_ACT;
  if (!c->pre_ln) {
    const float hidden_drop = keep ? c->hidden_drop : 0.f, attn_drop = keep ? c->attn_drop : 0.f;
    const uint32_t seed = keep ? c->seed : 0u, attn_seed = keep ? c->seed * 2654435761u + c->layer_id * 97u + 17u : 0u;
    const uint32_t ln1_stream = keep ? c->layer_id * 4u + 0u : 0u, ln2_stream = keep ? c->layer_id * 4u + 1u : 0u;
    // Both promises of masked_rows_dead (padded rows, a key mask): nobody reads this layer's output at a masked position.  Such a row is a
    // masked key of every attention (P = 0 exactly), no head reads it, and its incoming gradient is exactly zero, so whatever the stash
    // holds for it meets an exact zero in every weight-gradient sum: its values may be anything finite.  The GEMMs run the 32-row blocks
    // that hold a live row only (one block list per call, or the caller's), the LayerNorms the live rows only (dead rows leave as zeros).
    // Zeros are written where somebody reads every row: q / k / v (the attention kernels), the FFN activation and its derivative (the
    // fc2 weight gradient's partly live 32-row blocks, the every-row x gelu' epilogue).  The two projection outputs in front of the LayerNorms
    // are not filled: only their LayerNorm reads them, which skips the dead rows and, in the training form, overwrites them in place.
    // ... and the GEMMs whose slab form exists take the mask in 8-row slabs (ia_row_slabs: a sequence's rows never line up with 32-row
    // blocks).  The same readers, the same argument: a dead slab of a live block holds zeros where a dead block does, and is unwritten
    // where a dead block is (the two projection outputs).  (The forward-only activation epilogue has no slab form: it keeps the blocks.)
    RowPlan rows;
    const bool gate = (c->masked_rows_dead & IA_ROWS_DEAD_FWD) && (c->masked_rows_dead & IA_ROWS_DEAD_BWD) && g_fwd_rows;
    IA_TRY(resolve_rows(c, KEY_MASK, gate ? key_mask : nullptr, WANT_BLOCKS | WANT_SLABS, M, s.key, st, &rows));
    // qkv = x Wqkv^T + b
    IA_TRY(qkv_proj(c, x, w, s.qkv, M, scale, st, rows.slabs));
    IA_TRY(attn_fwd(c, s.qkv, key_mask, s.ctx, s.lse, scale, attn_drop, attn_seed, st));
    // out_row_live: behind the attention only the rows the caller reads are live (a subset of the live keys) -- the same rules with that
    // mask and its block list: the LayerNorms leave zeros in the other rows (so y1 and, in the training form, z1 / z2 are finite in every
    // row a partly live 32-row block of a weight gradient touches), fc1 fills the other blocks of the activation and its derivative
    // (out_row_live keeps its 32-row lists)
    if (const uint8_t* const olive = out_live(c)) IA_TRY(resolve_rows(c, OUT_ROWS, olive, WANT_BLOCKS, M, s.out, st, &rows));
    // z1 = x + dropout(ctx Wo^T + b_o); y1 = LN1(z1)
    IA_TRY(fwd_gemm(s.ctx, H, w->w_o, s.proj, H, M, IA_EPI_NONE, nullptr, nullptr, nullptr, rows, false, st));
    IA_TRY(ia_ln_fwd_rows(s.proj, w->b_o, x, keep ? s.proj : nullptr, s.ln, s.mean1, s.rstd1, w->ln1_g, w->ln1_b, M, H, c->eps, hidden_drop, seed,
                          ln1_stream, rows.live, st));
    // h = gelu(y1 W1^T + b1)
    IA_TRY(fwd_gemm(s.ln, H, w->w_fc1, s.hact, I, M, gelu, w->b_fc1, nullptr, s.hpre, rows, true, st));
    // z2 = y1 + dropout(h W2^T + b2); y = LN2(z2)
    IA_TRY(fwd_gemm(s.hact, I, w->w_fc2, s.ffn, H, M, IA_EPI_NONE, nullptr, nullptr, nullptr, rows, false, st));
    IA_TRY(ia_ln_fwd_rows(s.ffn, w->b_fc2, s.ln, keep ? s.ffn : nullptr, y, s.mean2, s.rstd2, w->ln2_g, w->ln2_b, M, H, c->eps, hidden_drop, seed,
                          ln2_stream, rows.live, st));
  } else {   // no dropout (timm ViT default; ia_layer_fwd refuses it)
    IA_TRY(ia_ln_fwd(x, nullptr, nullptr, nullptr, s.xn, s.mean1, s.rstd1, w->ln1_g, w->ln1_b, M, H, c->eps, 0.f, 0, 0, st));
    IA_TRY(qkv_proj(c, s.xn, w, s.qkv, M, scale, st, IaRowFilter{}));
    IA_TRY(attn_fwd(c, s.qkv, key_mask, s.ctx, s.lse, scale, 0.f, 0, st));
    // x1 = x + ctx Wo^T + b_o and LN2(x1): the bias and the residual are added by the LayerNorm kernel (it streams the rows anyway),
    // so the projection keeps the plain epilogue; proj receives x1 in place of the raw projection (the fc2 epilogue's residual)
    // out_row_live (the last block under a head that reads [CLS] only): the out-projection, LN2, fc1 and fc2 run the 32-row blocks / rows
    // the caller reads.  LN2 leaves zeros in the other rows of x1 and LN2(x1), fc1 fills the other blocks of the activation and its
    // derivative (the weight gradients' partly live 32-row blocks and the x gelu' epilogue read them); y is not written outside the live blocks.
    RowPlan rows;
    IA_TRY(resolve_rows(c, OUT_ROWS, out_live(c), WANT_BLOCKS, M, s.out, st, &rows));
    IA_TRY(fwd_gemm(s.ctx, H, w->w_o, s.proj, H, M, IA_EPI_NONE, nullptr, nullptr, nullptr, rows, false, st));
    IA_TRY(ia_ln_fwd_rows(s.proj, w->b_o, x, s.proj, s.ln, s.mean2, s.rstd2, w->ln2_g, w->ln2_b, M, H, c->eps, 0.f, 0, 0, rows.live, st));
    IA_TRY(fwd_gemm(s.ln, H, w->w_fc1, s.hact, I, M, gelu, w->b_fc1, nullptr, s.hpre, rows, true, st));
    IA_TRY(fwd_gemm(s.hact, I, w->w_fc2, y, H, M, IA_EPI_BIAS_ADD, w->b_fc2, s.proj, nullptr, rows, false, st));
  }

  return IA_OK;
}

}  // namespace

extern "C" int ia_debug_fwd_rows(int on) {
  const int was = g_fwd_rows;
  g_fwd_rows = on ? 1 : 0;
  return was;
}

extern "C" int ia_debug_out_rows(int on) {
  const int was = g_out_rows;
  g_out_rows = on ? 1 : 0;
  return was;
}

extern "C" int ia_debug_q_rows(int on) {
  const int was = g_q_rows;
  g_q_rows = on ? 1 : 0;
  return was;
}

extern "C" int ia_debug_dgrad_rows(int on) {
  const int was = g_dgrad_rows;
  g_dgrad_rows = on ? 1 : 0;
  return was;
}

extern "C" size_t ia_layer_stash_bytes(const ia_layer_cfg* cfg) {
  (void)hipGetLastError();  // drop stale status left by unrelated runtime calls (e.g. hipEventQuery -> NotReady)
  if (!cfg_ok(cfg)) return 0;
  return carve_stash(cfg, nullptr).bytes;
}

extern "C" size_t ia_layer_bwd_scratch_bytes(const ia_layer_cfg* cfg) {
  (void)hipGetLastError();  // drop stale status left by unrelated runtime calls (e.g. hipEventQuery -> NotReady)
  if (!cfg_ok(cfg)) return 0;
  return carve_scratch(cfg, nullptr).bytes;
}

extern "C" size_t ia_layer_infer_scratch_bytes(const ia_layer_cfg* cfg) {
  (void)hipGetLastError();
  if (!cfg_ok(cfg)) return 0;
  return carve_infer(cfg, nullptr).bytes;
}

extern "C" int ia_layer_fwd(const ia_layer_cfg* c, const ia_layer_weights* w, const void* x, const uint8_t* key_mask, void* y,
                            void* stash, ia_stream_t st) {
  (void)hipGetLastError();  // drop stale status left by unrelated runtime calls (e.g. hipEventQuery -> NotReady)
  if (!cfg_ok(c) || !w || !x || !y || !stash) return IA_ERR_ARG;
  if (c->pre_ln && (c->hidden_drop > 0.f || c->attn_drop > 0.f)) return IA_ERR_UNSUPPORTED;  // timm ViT default: no dropout
  return layer_forward(c, w, x, key_mask, y, carve_stash(c, stash), true, st);
}

// forward only, in a transient scratch that every layer of a stack can share
extern "C" int ia_layer_fwd_infer(const ia_layer_cfg* c, const ia_layer_weights* w, const void* x, const uint8_t* key_mask, void* y,
                                  void* scratch, size_t scratch_bytes, ia_stream_t st) {
  (void)hipGetLastError();
  if (!cfg_ok(c) || !w || !x || !y || !scratch) return IA_ERR_ARG;
  if (scratch_bytes < ia_layer_infer_scratch_bytes(c)) return IA_ERR_WORKSPACE;
  return layer_forward(c, w, x, key_mask, y, carve_infer(c, scratch), false, st);
}

extern "C" int ia_layer_bwd2(const ia_layer_cfg* c, const ia_layer_weights* w, const ia_layer_grads* g, const void* x,
                             const uint8_t* key_mask, const void* y, const void* stash, const void* dy, const void* dy2, void* dx, void* dx2,
                             void* scratch, size_t scratch_bytes, ia_stream_t st);

extern "C" int ia_layer_bwd(const ia_layer_cfg* c, const ia_layer_weights* w, const ia_layer_grads* g, const void* x,
                            const uint8_t* key_mask, const void* y, const void* stash, const void* dy, void* dx, void* scratch,
                            size_t scratch_bytes, ia_stream_t st) {
  return ia_layer_bwd2(c, w, g, x, key_mask, y, stash, dy, nullptr, dx, nullptr, scratch, scratch_bytes, st);
}

extern "C" int ia_layer_bwd2(const ia_layer_cfg* c, const ia_layer_weights* w, const ia_layer_grads* g, const void* x,
                             const uint8_t* key_mask, const void* y, const void* stash, const void* dy, const void* dy2, void* dx, void* dx2,
                             void* scratch, size_t scratch_bytes, ia_stream_t st) {
  (void)hipGetLastError();  // drop stale status left by unrelated runtime calls (e.g. hipEventQuery -> NotReady)
  (void)y;
  if (!cfg_ok(c) || !w || !g || !x || !stash || !dy || !dx || !scratch) return IA_ERR_ARG;
  if (c->pre_ln && (dy2 || dx2)) return IA_ERR_UNSUPPORTED;
  if (scratch_bytes < ia_layer_bwd_scratch_bytes(c)) return IA_ERR_WORKSPACE;
  const int M = (int)rows_of(c), H = c->H, I = c->I;
  const FwdBufs s = carve_stash(c, const_cast<void*>(stash));
  const Scratch k = carve_scratch(c, scratch);
  const float scale = 0.125f;
  const uint32_t attn_seed = c->seed * 2654435761u + c->layer_id * 97u + 17u;
  const bool drop = c->hidden_drop > 0.f;
  // out_row_live: the incoming gradient is zero outside these rows, so every gradient in front of the attention backward is too.  Its
  // block mask, block list and group list (the caller's, or built here) filter the kernels from the LN2 backward to the out-projection's
  // gradients; the attention backward and the QKV gradients keep the layer's other filter (every row is a key).
  // The weight gradients walk the live 16-row steps of k where the shape allows (ia_gemm_wgrad_walk), from a step mask this call builds
  // in its scratch (one small launch per mask), else the live 32-row blocks of the caller's block mask or one built here.
  const int behind_attn[3][2] = {{H, I}, {I, H}, {H, H}}, qkv_shape[1][2] = {{3 * H, H}};
  RowPlan out;
  IA_TRY(resolve_rows(c, OUT_ROWS, out_live(c), want_wgrad_masks(behind_attn, 3, M) | WANT_BLOCKS | WANT_GROUPS, M, k.out, st, &out));
  if (!c->pre_ln) {
    // masked_rows_dead: every gradient row of a masked position is exactly zero (ia_layer_cfg): the LayerNorm backward kernels skip them,
    // the four weight gradients skip the 16-row steps of k that hold nothing else (32-row blocks where the k-slab is too long), the two
    // plain data gradients behind the attention and the QKV one run the live 8-row slabs (their dead rows are written as zeros: the
    // attention backward, the pair kernels and the embedding backward read every row), and the x gelu' + column-sums data gradient the
    // live blocks packed by whole 128-row groups.  ia_debug_dgrad_rows withholds the lists of the data gradients, not the mask.
    RowPlan key;
    const unsigned key_masks = want_wgrad_masks(qkv_shape, 1, M) | (out.live ? 0u : want_wgrad_masks(behind_attn, 3, M));
    IA_TRY(resolve_rows(c, KEY_MASK, key_mask, key_masks | (g_dgrad_rows ? WANT_PACKED | WANT_SLABS : 0), M, k.key, st, &key));
    // behind the attention: out_row_live's plan when given (a subset of the live keys), else the key mask's
    const RowPlan& rows = out.live ? out : key;
    // The two residual additions of a post-LN layer make each LayerNorm output's gradient a sum of two terms; both LayerNorm
    // backward kernels take the two terms (ia_ln_bwd2), so the GEMMs in front of them keep the plain epilogue.
    // LN2 backward: d(output) = dy (+ dy2) -> dz2 in g0, masked branch gradient -> g1 (or g0 when p == 0)
    IA_TRY(ia_ln_bwd2_rows(dy, dy2, nullptr, s.ffn, s.mean2, s.rstd2, w->ln2_g, k.g0, drop ? k.g1 : nullptr, g->ln2_g, g->ln2_b, g->b_fc2, M, H,
                           c->hidden_drop, c->seed, c->layer_id * 4u + 1u, rows.live, k.ws, k.ws_bytes, 1, st));
    const char* d_ffn = drop ? k.g1 : k.g0;
    IA_TRY(wgrad(d_ffn, H, s.hact, I, (float*)g->w_fc2, M, rows, k.gws, k.gws_bytes, st));
    // d(pre-activation) = (d_ffn W2) * gelu'(pre), and its column sums (the fc1 bias gradient) out of the same epilogue
    IA_TRY(dgrad(d_ffn, H, w->w_fc2, w->wt_fc2, I, k.gI, M, IA_EPI_DGELU_COLSUM, s.hpre, I, g->b_fc1, k.ws, k.ws_bytes, st, rows));
    IA_TRY(wgrad(k.gI, I, s.ln, H, (float*)g->w_fc1, M, rows, k.gws, k.gws_bytes, st));
    IA_TRY(dgrad(k.gI, I, w->w_fc1, w->wt_fc1, H, k.g2, M, IA_EPI_NONE, nullptr, 0, nullptr, nullptr, 0, st, rows));
    // LN1 backward: d(y1) = g2 (through fc1) + g0 (residual into LN2) -> dz1 (the layer input's residual-path gradient) in
    // dz1buf: the caller's dx2 when the split form is wanted, else g0 (in place over the term just consumed)
    char* dz1buf = dx2 ? (char*)dx2 : k.g0;
    IA_TRY(ia_ln_bwd2_rows(k.g2, k.g0, nullptr, s.proj, s.mean1, s.rstd1, w->ln1_g, dz1buf, drop ? k.g1 : nullptr, g->ln1_g, g->ln1_b, g->b_o, M, H,
                           c->hidden_drop, c->seed, c->layer_id * 4u + 0u, rows.live, k.ws, k.ws_bytes, 1, st));
    const char* d_att = drop ? k.g1 : dz1buf;
    IA_TRY(wgrad(d_att, H, s.ctx, H, (float*)g->w_o, M, rows, k.gws, k.gws_bytes, st));
    // (d_ctx and dz1 are zeros outside out_row_live: the attention backward and the QKV data gradient's "+ dz1" read every live key's row)
    IA_TRY(dgrad(d_att, H, w->w_o, w->wt_o, H, k.g2, M, IA_EPI_NONE, nullptr, 0, nullptr, nullptr, 0, st, rows));
    IA_TRY(attn_bwd(c, s.qkv, key_mask, s.ctx, k.g2, s.lse, k.delta, k.gqkv, g->b_qkv, k.ws, k.ws_bytes, scale, c->attn_drop, attn_seed, st));
    IA_TRY(wgrad(k.gqkv, 3 * H, x, H, (float*)g->w_qkv, M, key, k.gws, k.gws_bytes, st));
    if (dx2)   // split form: dx = the attention sub-block's data gradient, dx2 = dz1 (already written)
      IA_TRY(dgrad(k.gqkv, 3 * H, w->w_qkv, w->wt_qkv, H, dx, M, IA_EPI_NONE, nullptr, 0, nullptr, nullptr, 0, st, key));
    else
      IA_TRY(dgrad(k.gqkv, 3 * H, w->w_qkv, w->wt_qkv, H, dx, M, IA_EPI_ADD, dz1buf, H, nullptr, nullptr, 0, st, key));
  } else {
    if (!c->dy_colsum_done) IA_TRY(ia_colsum(dy, H, M, H, g->b_fc2, 1, k.ws, k.ws_bytes, st));
    // (without out_row_live the plan is empty: the helpers then make the plain every-row calls)
    IA_TRY(wgrad(dy, H, s.hact, I, (float*)g->w_fc2, M, out, k.gws, k.gws_bytes, st));
    IA_TRY(dgrad(dy, H, w->w_fc2, w->wt_fc2, I, k.gI, M, IA_EPI_DGELU_COLSUM, s.hpre, I, g->b_fc1, k.ws, k.ws_bytes, st, out));
    IA_TRY(wgrad(k.gI, I, s.ln, H, (float*)g->w_fc1, M, out, k.gws, k.gws_bytes, st));
    IA_TRY(dgrad(k.gI, I, w->w_fc1, w->wt_fc1, H, k.g0, M, IA_EPI_NONE, nullptr, 0, nullptr, nullptr, 0, st, out));
    // LN2 backward (+ residual path dy) -> g1 = d x2 ; its column sum is the proj-bias gradient
    // (the row-filtered launch keeps every row's place in the partial sums: leaving out rows that add exact zeros changes no bit)
    IA_TRY(ia_ln_bwd2_rows(k.g0, nullptr, dy, s.proj, s.mean2, s.rstd2, w->ln2_g, k.g1, nullptr, g->ln2_g, g->ln2_b, g->b_o, M, H, 0.f, 0, 0, out.live,
                           k.ws, k.ws_bytes, 1, st));
    IA_TRY(wgrad(k.g1, H, s.ctx, H, (float*)g->w_o, M, out, k.gws, k.gws_bytes, st));
    IA_TRY(dgrad(k.g1, H, w->w_o, w->wt_o, H, k.g2, M, IA_EPI_NONE, nullptr, 0, nullptr, nullptr, 0, st, out));
    IA_TRY(attn_bwd(c, s.qkv, key_mask, s.ctx, k.g2, s.lse, k.delta, k.gqkv, g->b_qkv, k.ws, k.ws_bytes, scale, 0.f, 0, st));
    IA_TRY(wgrad(k.gqkv, 3 * H, s.xn, H, (float*)g->w_qkv, M, RowPlan{}, k.gws, k.gws_bytes, st));
    IA_TRY(dgrad(k.gqkv, 3 * H, w->w_qkv, w->wt_qkv, H, k.g0, M, IA_EPI_NONE, nullptr, 0, nullptr, nullptr, 0, st, RowPlan{}));
    // dx = LN1'(g0) + g1 is the incoming gradient of the block below: its column sums (that block's fc2 bias gradient) come out of
    // this kernel's partial sums instead of a separate pass over [M, H] there (cfg->dx_colsum_out)
    IA_TRY(ia_ln_bwd(k.g0, k.g1, x, s.mean1, s.rstd1, w->ln1_g, dx, nullptr, g->ln1_g, g->ln1_b, c->dx_colsum_out, M, H, 0.f, 0, 0, k.ws,
                     k.ws_bytes, 1, st));
  }

  return IA_OK;
}
