// bf16 MFMA GEMM for the encoder hot path (gfx950).
//
//   C[M,N] = A[M,K] * B[K,N]   (+ fused epilogue), fp32 accumulate in MFMA accumulators.
//
// Operand memory layouts (no explicit transposes anywhere on the path):
//   A k-contiguous : A[m][k]  (activations / output-gradients, row = token)
//   A k-strided    : At[k][m] (dW = dY^T X : the "A" of that product is dY stored [token][n])
//   B k-contiguous : Bt[n][k] (a torch Linear weight W[N,K] used in the forward)
//   B k-strided    : B[k][n]  (the same W used for dX = dY W, and X in dW = dY^T X)
// k-strided operands are staged row-major into LDS exactly as they lie in HBM and are turned into
// MFMA fragments with ds_read_b64_tr_b16 (the LDS transpose read), so the reference's three GEMM
// flavours (y = xW^T, dx = dy W, dW = dy^T x; torch.nn.Linear under autograd, reference
// src/models/text.py:1241 -> transformers RobertaLayer) all stream each operand from HBM once.
//
// Two tile configurations (make_plan chooses by output size):
//   T256W: 256x256x64 per 256-thread workgroup (4 waves as 2x2, one per SIMD, 128x128 per wave, 4x4 MFMA 32x32x16
//          fragments, 128 KiB LDS double buffer), persistent over output tiles - the large-M encoder GEMMs.  T256LA is
//          its plain-NT variant whose k pipeline runs on into the next tile.
//   T128:  128x128x64 per 256-thread workgroup (4 waves as 2x2, 64x64 per wave, 4x4 MFMA 16x16x32) -
//          small outputs (heads, tiny test shapes), the shifted-view convolution GEMMs and channel groups.
// LDS is filled by buffer_load ... lds (16 B/lane; out-of-range rows arrive as zeros, so ragged M / K
// tails need no extra code) with the XOR swizzle applied on the source side.  The MFMA is issued with
// swapped operands (C^T fragments) so each lane ends up with runs of consecutive output columns.
#include "common.h"
#include <atomic>
#include <cstdlib>
#include <type_traits>

// The IA_GEMM_DBG timing ablations (switching the DMA, the barriers, the epilogue, its stores or its math off) exist in tools builds
// only (-DIA_GEMM_DBG_HOOKS=1): left in as run-time tests they put a branch around every GELU pair of the FFN1 epilogue (334 branches
// and 1882 s_nops in that kernel: each pair in its own basic block, the four independent chains of a call never interleaved).
#ifndef IA_GEMM_DBG_HOOKS
#define IA_GEMM_DBG_HOOKS 0
#endif
#define IA_DBG(p) (IA_GEMM_DBG_HOOKS ? (p).dbg : 0)

namespace {

constexpr int BK = 64;
constexpr uint32_t OOB = 0xFFFFFFF0u;

enum { EPI_NONE = 0, EPI_BIAS = 1, EPI_BIAS_GELU = 2, EPI_ADD = 3, EPI_DGELU = 4, EPI_BIAS_ADD = 5, EPI_DGELU_CS = 6, EPI_BIAS_GELU_ACT = 7 };
// EPI_NONE_BLK (library-internal, t256w only): EPI_NONE behind a k loop over the live 32-row blocks.  The weight-gradient form
// dW = dY^T X has the token rows as k: a block whose rows of dY are all zeros adds +-0 to every accumulator, so leaving it out changes
// no bit of the fp32 sums -- the k-slabs of a split-K launch and the order of the reduction stay what they are, a slab just takes fewer
// trips.  A k-tile of the loop is made of TWO live 32-row blocks of the slab, the next one of the ascending walk in its lower half (LDS
// rows 0 .. 31: DMA pieces 0 .. 3, k-steps 0 and 1) and the one after it in its upper half (pieces 4 .. 7, k-steps 2 and 3).  A 32-row
// block is two whole 32x32x16 MFMAs per accumulator, so every accumulator still sees the MFMAs of its live rows on the same operands in
// the same order, less those whose dY operand is all zeros, and a slab takes ceil(live blocks / 2) trips.  (The value 8 was the walk
// over whole 64-row k-tiles this one replaced; 9 stays, and with it the kernel's name in the profiles.)
constexpr int EPI_NONE_BLK = 9;
// EPI_NONE_STP (library-internal, t256w only): the same walk over the live 16-row STEPS of an ia_kstep_mask, FOUR to a k-tile.  A 16-row
// step is one whole 32x32x16 MFMA per accumulator, so the argument above holds unchanged: step q of a trip is DMA pieces 2q and 2q + 1
// (LDS rows 16q .. 16q + 15) and k-step q, and a slab takes ceil(live steps / 4) trips.  A 32-row block with one live row costs a whole
// block under the block walk and half of one here (0.60-0.62 of the rows against 0.66-0.68 at the benchmark's lengths).  The slab's bits
// are one word per lane, four per k-tile: slabs of up to 512 k-tiles (step_mask_fits); longer ones keep the block walk.
constexpr int EPI_NONE_STP = 10;
// EPI_ROWS + e (library-internal, t256w only; k-contiguous A, bf16 output): epilogue e behind a row remap.  The data gradient dX = dY W
// (e = EPI_NONE, EPI_ADD or EPI_DGELU_CS) has the token rows as M: a row of dY that is all zeros gives a row of zeros, so only the 32-row
// blocks that hold a live row are computed -- an M-tile is eight consecutive entries of the live-block list (GemmArgs::row_blk) instead
// of 256 consecutive rows -- and the dead blocks are written as zeros by a fill launch.  No live row's arithmetic changes.
// The forward forms (e = EPI_NONE, EPI_BIAS with qcols / qscale, EPI_BIAS_GELU with both outputs, EPI_BIAS_GELU_ACT, EPI_BIAS_ADD; both
// operands k-contiguous) skip the blocks whose rows nobody reads (padded positions under ia_layer_cfg::masked_rows_dead bit 2); there the fill is
// the caller's choice (GemmArgs::rows_fill): without it the dead blocks of C / C2 are not written at all.
constexpr int EPI_ROWS = 16;
// EPI_ROWS + EPI_SLABS + e (library-internal; e = EPI_NONE, EPI_ADD, and on k-contiguous operands EPI_BIAS, EPI_BIAS_GELU): the same remap in
// 8-row slabs.  GemmArgs::row_blk is a list ia_row_slabs wrote; an M-tile is 32 consecutive entries of it.  A DMA piece is 32 rows of
// which wave w carries rows 8w .. 8w+7, so each wave hands its own slab to each piece (eight scalars per wave, where the block form has
// eight per workgroup); the epilogue stores in passes of 8 whole rows, one slab each (sixteen scalars per wave).  Slabs are aligned to
// multiples of 8 rows of the tensor and never overlap: no row is computed, stored or summed twice, and no live row's arithmetic changes.
constexpr int EPI_SLABS = 32;
// EPI_BIAS_GELU_ACT: the forward-only form of EPI_BIAS_GELU (activation only: no derivative is evaluated or stored)

struct GemmArgs {
  const bf16* A; const bf16* B; void* C; bf16* C2;
  union {
    const float* bias;
    // Weight-gradient form of the 256-wide kernel only (IA_EPI_NONE: no bias; the member shares its slot so that no other kernel's
    // argument block moves): bit t of this bitmask (an ia_kblock_mask) set = block t (k rows 32t .. 32t+31) has at least one row of A that
    // is not known to be all zeros; a workgroup walks only the set bits of its k-slab (t256w::gemm_kernel<true, true, EPI_NONE_BLK, true>).
    // NULL = every row.
    const uint32_t* live_blk;
  };
  const bf16* aux;
  int M, N, K;
  int lda, ldb, ldc, ldaux;
  uint64_t a_bytes, b_bytes;  // bytes addressable from A / B (to the end of the tensor); each workgroup re-bases a < 2 GiB buffer window inside them
  int accumulate;
  // IA_EPI_BIAS only: columns n < qcols leave as (acc + bias) * qscale -- the fused QKV projection hands the attention kernels
  // q * (softmax scale * log2 e), rounded to bf16 ONCE, so that forward, dQ, dK/dV and the fused backward exponentiate identical
  // products without any of them re-scaling q (ia_gemm_bf16_qscale); 0 = off
  int qcols; float qscale;
  int tiles_m, tiles_n;
  int splits, nk_per_split;   // split-K (fp32 output only): split s owns k-tiles [s*nk_per_split, ...)
  float* csum_part;           // EPI_DGELU_CS: [ceil(M/128)][N] fp32 column sums of each 128-row block of the output (256-wide kernels only)
  int split_id;               // set inside the kernels (derived from the XCD-aware work order)
  float* ws;                  // [splits][M][N] fp32 partials when splits > 1
  // weight-gradient form (A, B k-strided, fp32 C), T128: rsum_out[group * M + m] += sum_k A[k][m] -- the bias gradient of the layer,
  // taken from the A tiles already in LDS by one more MFMA against a fragment of ones (no second pass over dy).
  float* rsum_out;            // NULL = off
  float* rsum_ws;             // [groups][splits][M] partials when splits > 1 (folded by the split-K reduce kernels)
  int dbg;                    // ablation switches for tuning runs (IA_GEMM_DBG env): results are WRONG when non-zero
  // Shifted operand views (T128 only) that turn the GEMM into a 3x3 convolution over a zero-bordered NHWC tensor
  // [B, H+2, W+2, C] without a patch matrix: the k axis is (tap, channel) with a power-of-two channel count per tap, and tap t
  // reads the same rows shifted by tap_delta(t) = (t/3 - 1) * pw + (t%3 - 1).
  //   a_view +1 / -1 (k-contiguous A): k = (tap << lca) + ch reads row + / - tap_delta(tap), column ch        (forward / data grad)
  //   b_view 1 (k-strided B = W[o][(tap << lcbn) + c]): k = (tap << lcbk) + o, column n reads W[o][(tap << lcbn) + n]   (data grad)
  //   b_view 2 (k-strided B = the activations): column n = (tap << lcbn) + ch reads row k + tap_delta(tap), column ch  (weight grad)
  int a_view, b_view, pw, lca, lcbk, lcbn;
  // channel groups: operands advance by ga / gb / gc / gbias elements per group (all groups in one launch)
  int groups;
  long ga, gb, gc, gbias;
  // Dynamic tile claim (t256w, persistent launches): 8 per-XCD claim counters + 1 exit counter of this launch's slot (zero on entry,
  // zeroed again by the last workgroup to leave); NULL = the static order (tile + gridDim.x).
  uint32_t* tile_ctr;
  // Row-remapped form of the 256-wide kernels only (EPI_ROWS + e): the block list ia_row_blocks wrote, NULL = every row.  Behind every
  // member the other kernels read, so their argument blocks keep their layout.  rows_fill (host side): the launch writes the dead
  // blocks' rows of C (and C2) as zeros first.
  const int* row_blk;
  int rows_fill, fill_m;      // fill_m: the rows the fill covers (M, unless the remapped launch leaves its last rows to a launch of their own)
  // EPI_ROWS + EPI_BIAS: every wave takes the row-layout epilogue, (acc + bias) * qscale -- the launch over the rows behind the last whole
  // 128-row part of M, which the dense kernel rounds that way (gemm_core)
  int rows_guarded;
  // EPI_ROWS + EPI_DGELU_CS: the list is group-aligned (ia_row_groups: entries 4i .. 4i+3 are the four 32-row blocks of ONE 128-row group,
  // so a wave's four block slots are one group in order) and the wave writes its column-sum partial to THAT group's slot of csum_part,
  // where the dense kernel puts it: the second stage then adds the same fp32 terms in the same places (dead groups' slots are zeroed)
  // 2: the list is block-packed (ia_row_groups_packed): a wave's four slots hold the live blocks of one or more whole groups, each group's
  // blocks contiguous and ascending, empty slots (-1) behind them.  The wave folds and stores its column sums where the group changes,
  // into that group's slot, and starts the next group from zero: a lane adds the rows of a group's live blocks in the dense kernel's
  // order with nothing in between (the blocks left out added +-0 there), so every partial keeps its bits.  The fill zeroes all slots.
  int rows_grouped;
};

// One slot per launch in flight (launches of different streams may overlap; a slot comes round again after CTR_SLOTS launches).
constexpr int CTR_SLOTS = 1024, CTR_WORDS = 16;
__device__ uint32_t g_tile_ctr[CTR_SLOTS * CTR_WORDS];

IA_DEV int tap_delta(int t, int pw) { return (t / 3 - 1) * pw + (t % 3 - 1); }

// Buffer window that starts `origin` elements into an operand of `total_bytes` bytes.  Buffer offsets are 32-bit, operands (an
// 800x800 feature map of 64 images, a 9x patch matrix) are not: every workgroup addresses its tile / k-slab relative to its own
// origin, and the range check still ends at the end of the tensor (lanes past it read zeros).
IA_DEV __amdgpu_buffer_rsrc_t rsrc_at(const bf16* base, uint64_t total_bytes, uint64_t origin) {
  const uint64_t ob = origin * 2, rem = total_bytes > ob ? total_bytes - ob : 0;
  return ia_rsrc(base + origin, (uint32_t)(rem < 0x7FFFFFF0ull ? rem : 0x7FFFFFF0ull));
}

// ---------------------------------------------------------------------------------- shared epilogue
// v = 4 consecutive output columns n..n+3 of row m
template <int EPI, bool OUTF32>
IA_DEV void epi_store4(const GemmArgs& p, int m, int n, f32x4 v) {
  if (EPI == EPI_BIAS || EPI == EPI_BIAS_GELU || EPI == EPI_BIAS_GELU_ACT || EPI == EPI_BIAS_ADD) {
    const f32x4 b = *reinterpret_cast<const f32x4*>(p.bias + n);
    v += b;
    if (EPI == EPI_BIAS && n < p.qcols) v *= p.qscale;
  }
  if (EPI == EPI_BIAS_GELU) {
    // C = gelu(pre), C2 = gelu'(pre): the derivative shares the exp / rcp of the activation (gelu_pair, common.h) and turns the
    // data-gradient epilogue (EPI_DGELU) into one multiply per element
    bf16x4 der;
#pragma unroll
    for (int r = 0; r < 4; r += 2) {
      f32x2_t a, d;
      gelu_pair(f32x2_t{v[r], v[r + 1]}, a, d);
      v[r] = a[0]; v[r + 1] = a[1];
      der[r] = f2bf(d[0]); der[r + 1] = f2bf(d[1]);
    }
    *reinterpret_cast<bf16x4*>(p.C2 + (size_t)m * p.ldc + n) = der;
  }
  if (EPI == EPI_BIAS_GELU_ACT) {
#pragma unroll
    for (int r = 0; r < 4; r += 2) {
      const f32x2_t a = gelu_act_pair(f32x2_t{v[r], v[r + 1]});
      v[r] = a[0]; v[r + 1] = a[1];
    }
  }
  if (EPI == EPI_ADD || EPI == EPI_BIAS_ADD) {
    const bf16x4 a = *reinterpret_cast<const bf16x4*>(p.aux + (size_t)m * p.ldaux + n);
#pragma unroll
    for (int r = 0; r < 4; ++r) v[r] += bf2f(a[r]);
  }
  if (EPI == EPI_DGELU || EPI == EPI_DGELU_CS) {   // aux = the saved gelu'(pre-activation); T128 leaves the column sums to ia_colsum
    const bf16x4 a = *reinterpret_cast<const bf16x4*>(p.aux + (size_t)m * p.ldaux + n);
#pragma unroll
    for (int r = 0; r < 4; ++r) v[r] *= bf2f(a[r]);
  }
  if (OUTF32) {
    if (p.splits > 1) {   // partial sums; the second-stage kernel adds them into C in a fixed order
      *reinterpret_cast<f32x4*>(p.ws + ((size_t)p.split_id * p.M + m) * p.N + n) = v;
      return;
    }
    float* c = reinterpret_cast<float*>(p.C) + (size_t)m * p.ldc + n;
    if (p.accumulate) { const f32x4 o = *reinterpret_cast<const f32x4*>(c); v += o; }
    *reinterpret_cast<f32x4*>(c) = v;
  } else {
    bf16x4 o = {f2bf(v[0]), f2bf(v[1]), f2bf(v[2]), f2bf(v[3])};
    *reinterpret_cast<bf16x4*>(reinterpret_cast<bf16*>(p.C) + (size_t)m * p.ldc + n) = o;
  }
}

// One 16-byte global store = one VMEM instruction (hipcc emits a single global_store_dwordx4 for an aligned 16-byte vector store;
// tools/check_gemm_isa.sh counts them).  The persistent 256-wide kernels leave a tile's output stores in flight while the next tile's
// main loop starts and wait with a COUNTED s_waitcnt vmcnt(N) for the k-tile DMA issued before them (vmcnt retires in order), so
// the number of store instructions per epilogue must be known exactly.  The store is a plain (compiler-visible) one on purpose: the
// epilogue's aux / bias loads are software-pipelined two slices ahead of the stores, and only when hipcc counts the stores too does
// it wait for such a load with vmcnt(k > 0) and leave the younger stores in flight (an asm store is invisible to its counters: every
// load wait became vmcnt(0), i.e. a full store + load round trip per 8-row slice, 16 times per tile).
template <typename V>
IA_DEV void gstore16(void* ptr, V v) {
  static_assert(sizeof(V) == 16, "16-byte store");
  *reinterpret_cast<V*>(ptr) = v;      // (a non-temporal store measured the same: tools/README.md, GEMM ablations)
}
template <int EPI, bool OUTF32>
constexpr int epi_stores_per_call() { return OUTF32 ? 2 : (EPI == EPI_BIAS_GELU ? 2 : 1); }
template <int EPI>
constexpr int epi_extra_stores() { return EPI == EPI_DGELU_CS ? 2 : 0; }     // the wave's column-sum partial: two 16-byte stores

// v = 8 consecutive output columns n..n+7 of row m (row-coalesced epilogue of the 256-wide kernels).  PRE: bias (pb0 | pb1) and aux (ax)
// were fetched ahead by the caller; else they are loaded here.
// BUF (full tiles of the one-wave-per-SIMD kernel, bf16 outputs): the output streams are addressed through buffer windows over the
// wave's rows with one 32-bit lane offset (io.off) instead of 64-bit pointer arithmetic per access (3 VALU instructions each)
struct BufIO { __amdgpu_buffer_rsrc_t rsC, rsC2; uint32_t off; };
// PIN (the remapped x gelu' + column-sums forms): the column-sum arithmetic written out the way the compiled DENSE kernel does it, which
// differs between its two epilogue paths -- prefetched (full tiles): the product is rounded, then added; guarded (edge tiles): one fused
// multiply-add -- so that a group's partial keeps its bits wherever the remap puts the group, as long as it takes the path the dense
// kernel gives it (left to the compiler, the remapped kernel fused some of its prefetched slices and not others).
template <int EPI, bool OUTF32, bool PRE, bool BUF = false, bool PIN = false>
IA_DEV void epi_store8(const GemmArgs& p, int m, int n, f32x4 lo, f32x4 hi, f32x4 pb0, f32x4 pb1, bf16x8 ax, float (&cs)[8], const BufIO* io = nullptr) {
  float v[8] = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
  if (EPI == EPI_BIAS || EPI == EPI_BIAS_GELU || EPI == EPI_BIAS_GELU_ACT || EPI == EPI_BIAS_ADD) {
    const f32x4 b0 = PRE ? pb0 : *reinterpret_cast<const f32x4*>(p.bias + n), b1 = PRE ? pb1 : *reinterpret_cast<const f32x4*>(p.bias + n + 4);
#pragma unroll
    for (int r = 0; r < 4; ++r) { v[r] += b0[r]; v[4 + r] += b1[r]; }
    if (EPI == EPI_BIAS && n < p.qcols) {
#pragma unroll
      for (int r = 0; r < 8; ++r) v[r] *= p.qscale;
    }
  }
  if (EPI == EPI_BIAS_GELU) {   // see epi_store4
    bf16x8 der;
    {
      // the four pairs of the call stage by stage (gelu_pair's arithmetic, common.h): four independent chains side by side, so the
      // transcendental / packed-op latencies of one hide behind the others (one pair at a time left ~1.8 s_nops per exp2 / rcp)
      constexpr float L2E = 1.4426950408889634f;
      constexpr float C0 = 1.5949398799788077f, C1 = 0.07403000634661838f, C2 = -0.0007007124749191571f;
      constexpr float U_MAX = C1 / (2.f * 0.0007007124749191571f);
      f32x2_t x[4], u[4], t[4], e[4], sg[4], act[4], q[4], d[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) { x[i] = f32x2_t{v[2 * i], v[2 * i + 1]}; u[i] = x[i] * x[i]; }
#pragma unroll
      for (int i = 0; i < 4; ++i) { u[i][0] = __builtin_fminf(u[i][0], U_MAX); u[i][1] = __builtin_fminf(u[i][1], U_MAX); }
#pragma unroll
      for (int i = 0; i < 4; ++i) t[i] = x[i] * ((u[i] * (-C2 * L2E) + (-C1 * L2E)) * u[i] + (-C0 * L2E));
#pragma unroll
      for (int i = 0; i < 4; ++i) e[i] = f32x2_t{__builtin_amdgcn_exp2f(t[i][0]), __builtin_amdgcn_exp2f(t[i][1])};
#pragma unroll
      for (int i = 0; i < 4; ++i) { e[i] = e[i] + 1.0f; q[i] = (u[i] * (5.f * C2) + (3.f * C1)) * u[i] + C0; }
#pragma unroll
      for (int i = 0; i < 4; ++i) sg[i] = f32x2_t{__builtin_amdgcn_rcpf(e[i][0]), __builtin_amdgcn_rcpf(e[i][1])};
#pragma unroll
      for (int i = 0; i < 4; ++i) { act[i] = x[i] * sg[i]; d[i] = (act[i] * (1.0f - sg[i])) * q[i] + sg[i]; }
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        v[2 * i] = act[i][0]; v[2 * i + 1] = act[i][1];
        der[2 * i] = f2bf(d[i][0]); der[2 * i + 1] = f2bf(d[i][1]);
      }
    }
    if (BUF) __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, der), io->rsC2, (int)io->off, 0, 0);
    else gstore16(((IA_DBG(p) & 1024) ? reinterpret_cast<bf16*>(p.C) : p.C2) + (size_t)m * p.ldc + n, der);
  }
  if (EPI == EPI_BIAS_GELU_ACT) {      // gelu_act_pair's arithmetic, the four pairs stage by stage (see above)
    constexpr float L2E = 1.4426950408889634f;
    constexpr float C0 = 1.5949398799788077f, C1 = 0.07403000634661838f, C2 = -0.0007007124749191571f;
    constexpr float U_MAX = C1 / (2.f * 0.0007007124749191571f);
    f32x2_t x[4], u[4], t[4], e[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) { x[i] = f32x2_t{v[2 * i], v[2 * i + 1]}; u[i] = x[i] * x[i]; }
#pragma unroll
    for (int i = 0; i < 4; ++i) { u[i][0] = __builtin_fminf(u[i][0], U_MAX); u[i][1] = __builtin_fminf(u[i][1], U_MAX); }
#pragma unroll
    for (int i = 0; i < 4; ++i) t[i] = x[i] * ((u[i] * (-C2 * L2E) + (-C1 * L2E)) * u[i] + (-C0 * L2E));
#pragma unroll
    for (int i = 0; i < 4; ++i) e[i] = f32x2_t{__builtin_amdgcn_exp2f(t[i][0]), __builtin_amdgcn_exp2f(t[i][1])} + 1.0f;
    f32x2_t sg[4], act[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) sg[i] = f32x2_t{__builtin_amdgcn_rcpf(e[i][0]), __builtin_amdgcn_rcpf(e[i][1])};
#pragma unroll
    for (int i = 0; i < 4; ++i) act[i] = x[i] * sg[i];
#pragma unroll
    for (int i = 0; i < 4; ++i) { v[2 * i] = act[i][0]; v[2 * i + 1] = act[i][1]; }
  }
  if constexpr (EPI == EPI_DGELU_CS && PIN) {
    const bf16x8 a = PRE ? ax : *reinterpret_cast<const bf16x8*>(p.aux + (size_t)m * p.ldaux + n);
    if (PRE) {
#pragma clang fp contract(off)
#pragma unroll
      for (int r = 0; r < 8; ++r) { v[r] *= bf2f(a[r]); cs[r] += v[r]; }
    } else {
#pragma unroll
      for (int r = 0; r < 8; ++r) {
        const float x = v[r], y = bf2f(a[r]);
        v[r] = x * y;
        cs[r] = __builtin_fmaf(x, y, cs[r]);
      }
    }
  } else
  if (EPI == EPI_ADD || EPI == EPI_BIAS_ADD || EPI == EPI_DGELU || EPI == EPI_DGELU_CS) {
    const bf16x8 a = PRE ? ax : *reinterpret_cast<const bf16x8*>(p.aux + (size_t)m * p.ldaux + n);
#pragma unroll
    for (int r = 0; r < 8; ++r) {
      if (EPI == EPI_DGELU || EPI == EPI_DGELU_CS) v[r] *= bf2f(a[r]);
      else v[r] += bf2f(a[r]);
      if (EPI == EPI_DGELU_CS) cs[r] += v[r];       // this lane's 8 columns, summed over the rows it stores
    }
  }
  if (OUTF32) {
    float* c = p.splits > 1 ? p.ws + ((size_t)p.split_id * p.M + m) * p.N + n : reinterpret_cast<float*>(p.C) + (size_t)m * p.ldc + n;
    f32x4 o0 = {v[0], v[1], v[2], v[3]}, o1 = {v[4], v[5], v[6], v[7]};
    if (p.splits <= 1 && p.accumulate) { o0 += *reinterpret_cast<const f32x4*>(c); o1 += *reinterpret_cast<const f32x4*>(c + 4); }
    gstore16(c, o0);
    gstore16(c + 4, o1);
  } else {
    bf16x8 o;
#pragma unroll
    for (int r = 0; r < 8; ++r) o[r] = f2bf(v[r]);
    if (BUF) __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, o), io->rsC, (int)io->off, 0, 0);
    else gstore16(reinterpret_cast<bf16*>(p.C) + (size_t)m * p.ldc + n, o);
  }
}

// XCD-aware work order.  Workgroups are dealt round-robin to the 8 XCDs (each with a private L2): xcd_chunk renumbers them so that
// every XCD takes a contiguous run of the work list (bijective for any grid size) ...
IA_DEV int xcd_chunk(int bid, int nwg) {
  const int q = nwg >> 3, r = nwg & 7, xcd = bid & 7, idx = bid >> 3;
  return (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + idx;
}
// ... and the work list sweeps 8 m-tiles per n, so a run of 32 tiles is an 8 x 4 block: 8 A panels and 4 B panels feed 32 tiles
// out of one XCD's L2.
IA_DEV void tile_of_order(const GemmArgs& p, int t, int& bm, int& bn) {
  const int GM = 8;
  const int group = t / (GM * p.tiles_n);
  const int first_m = group * GM;
  const int gsz = min(p.tiles_m - first_m, GM);
  bm = first_m + (t % (GM * p.tiles_n)) % gsz;
  bn = (t % (GM * p.tiles_n)) / gsz;
}
IA_DEV void tile_of_index(const GemmArgs& p, int bid, int nwg, int& bm, int& bn) { tile_of_order(p, xcd_chunk(bid, nwg), bm, bn); }

// ============================================================================== T128 (4 waves, 16x16x32)
namespace t128 {
constexpr int BM = 128, BN = 128, TILE_BYTES = 16384;
// "row3" form of a shifted-view convolution GEMM (below): two 136-row A images + two B tiles; else two (A, B) k-tile pairs
constexpr int A3_ROWS = 136, A3_BYTES = A3_ROWS * 128, SMEM_BYTES = 2 * A3_BYTES + 2 * TILE_BYTES;
static_assert(SMEM_BYTES >= 4 * TILE_BYTES && 2 * SMEM_BYTES <= 160 * 1024, "two workgroups per CU");

// 32-byte-slot swizzle of a k-strided tile row (row = k index within the 64-row tile, 256 B rows)
IA_DEV int ks_swz(int k) { return ((k & 3) | (((k >> 3) & 1) << 2)) << 1; }

// x0 (k-contiguous) / korg (k-strided, views 0 and 2) are relative to the origin row of the buffer window `rs`
template <bool KS>
IA_DEV void stage_tile(__amdgpu_buffer_rsrc_t rs, char* s, int kt, int x0, int ld, int K, int tid, int wave, int korg, int view = 0, int pw = 0,
                       int lck = 6, int lcn = 6) {
#pragma unroll
  for (int issue = 0; issue < 4; ++issue) {
    uint32_t off;
    if (!KS) {
      const int row = issue * 32 + (tid >> 3);
      const int c = (tid & 7) ^ (row & 7);
      const int k = kt * BK + c * 8;
      if (view == 0) off = (uint32_t)(((x0 + row) * ld + k) * 2);
      else off = (uint32_t)(((x0 + row + view * tap_delta(k >> lck, pw)) * ld + (k & ((1 << lck) - 1))) * 2);   // rows before the tensor wrap to out-of-range
      if (k >= K) off = OOB;
    } else {
      const int row = issue * 16 + (tid >> 4);
      const int c = (tid & 15) ^ ks_swz(row);
      const int k = kt * BK + row;
      if (view == 0) off = (uint32_t)(((k - korg) * ld + x0 + c * 8) * 2);
      else if (view == 1) off = (uint32_t)(((k & ((1 << lck) - 1)) * ld + ((k >> lck) << lcn) + x0 + c * 8) * 2);
      else { const int col = x0 + c * 8; off = (uint32_t)(((k - korg + tap_delta(col >> lcn, pw)) * ld + (col & ((1 << lcn) - 1))) * 2); }
      if (k >= K) off = OOB;
    }
    __builtin_amdgcn_raw_ptr_buffer_load_lds(rs, IA_LDS(s + issue * 4096 + wave * 1024), 16, off, 0, 0, 0);
  }
}

IA_DEV bf16x8 frag_kc(const char* s, int row, int chunk) {
  return *reinterpret_cast<const bf16x8*>(s + row * 128 + ((chunk ^ (row & 7)) << 4));
}

IA_DEV bf16x8 frag_ks(const char* s, int k, int col) {
  // 16-lane group reads a [4 k][16 col] block twice (k, k+4); lane p supplies row k+(p>>2), 4 cols.
  const int addr = k * 256 + ((((col >> 3) ^ ks_swz(k))) << 4) + (col & 7) * 2;
  const uint32_t a = ia_lds_addr(s) + (uint32_t)addr;   // asm reads: the caller waits lgkmcnt(0) before the MFMAs
  s16x4 lo = ia_tr_read<0>(a);
  s16x4 hi = ia_tr_read<4 * 256>(a);
  s16x8 r = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
  return __builtin_bit_cast(bf16x8, r);
}

template <bool AKS, bool BKS, int EPI, bool OUTF32>
__global__ __launch_bounds__(256, 2) void gemm_kernel(GemmArgs p) {
  __shared__ __attribute__((aligned(16))) char smem[SMEM_BYTES];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave >> 1, wn = wave & 1;
  // 1-D grid over (k-slab, m-tile, channel group, n-tile), n-tile fastest, renumbered so that every XCD takes a contiguous run of it:
  // the work items that read the same rows of A -- the n-tiles of one slab (for a 3x3 weight gradient: its nine taps, i.e. nine
  // shifted views of the same rows) and the channel groups (128-byte column slices of the same rows) -- then run side by side on ONE
  // XCD and share its L2.  (As a 3-D grid they were dealt round-robin over the 8 XCDs and each XCD fetched the slab for itself.)
  int bm, bn, grp = 0;
  p.split_id = 0;
  if (p.groups > 1 || p.splits > 1) {
    int w = xcd_chunk(blockIdx.x, gridDim.x);
    bn = w % p.tiles_n; w /= p.tiles_n;
    grp = w % p.groups; w /= p.groups;
    bm = w % p.tiles_m;
    p.split_id = w / p.tiles_m;
  } else {
    tile_of_index(p, blockIdx.x, gridDim.x, bm, bn);
  }
  const int m0 = bm * BM, n0 = bn * BN;
  if (p.groups > 1) {                  // uniform: the kernel argument copy is ours to edit
    const long z = grp;
    p.A += z * p.ga; p.B += z * p.gb;
    p.a_bytes -= (uint64_t)(z * p.ga * 2); p.b_bytes -= (uint64_t)(z * p.gb * 2);     // the windows end where the tensors end
    p.C = reinterpret_cast<char*>(p.C) + z * p.gc * (OUTF32 ? 4 : 2);
    if (p.bias) p.bias += z * p.gbias;
    if (p.ws) p.ws += z * (long)p.splits * p.M * p.N;
  }

  f32x4 acc[4][4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  const int nk_all = (p.K + BK - 1) / BK;
  const int kt0 = p.split_id * p.nk_per_split;
  const int nk = min(nk_all, kt0 + p.nk_per_split);
  // buffer windows of this workgroup (rsrc_at): a k-contiguous operand starts at its tile's first row, a k-strided one at its
  // k-slab's first row, both moved back by the largest tap shift (pw + 1 rows) when the operand is read through shifted views
  const int a_org = !AKS ? max(0, m0 - (p.a_view ? p.pw + 1 : 0)) : kt0 * BK;
  const int b_org = !BKS ? n0 : (p.b_view == 1 ? 0 : max(0, kt0 * BK - (p.b_view == 2 ? p.pw + 1 : 0)));
  const __amdgpu_buffer_rsrc_t rsA = rsrc_at(p.A, p.a_bytes, (uint64_t)a_org * p.lda);
  const __amdgpu_buffer_rsrc_t rsB = rsrc_at(p.B, p.b_bytes, (uint64_t)b_org * p.ldb);
  const int xa = AKS ? m0 : m0 - a_org, xb = BKS ? n0 : 0;
  // ---- "row3": a 3x3 shifted-view convolution whose taps are whole k-tiles (64 channels per group: k-tile t = tap t) reads the SAME
  // 128 rows nine times, shifted by (dy, dx) rows.  The L2 -> LDS path is what bounds this kernel on those shapes (9 x the activation
  // bytes at the ~6.4 TB/s the chip's LDS-DMA engines sustain: 0.19 ms for 32 images x 200 x 200 x 64, measured), so the three taps of
  // one dy share ONE image of rows m0-1 .. m0+128 (136 rows fetched) and differ only in the LDS row their fragments start at: 3.2 x
  // the bytes instead of 9 x.  Forward and data gradient (a_view = +-1, k-contiguous A, N <= 64); the weight tiles stay per tap.
  const bool row3 = !AKS && p.a_view != 0 && p.lca == 6 && p.K == 9 * BK && p.splits == 1 && p.N <= 64;
  if (!row3) {
    stage_tile<AKS>(rsA, smem, kt0, xa, p.lda, p.K, tid, wave, a_org, p.a_view, p.pw, p.lca, 0);
    stage_tile<BKS>(rsB, smem + TILE_BYTES, kt0, xb, p.ldb, p.K, tid, wave, b_org, p.b_view, p.pw, p.lcbk, p.lcbn);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
  }

  const int g = lane >> 4, li = lane & 15;
  // A wave whose 64 x 64 quadrant lies entirely outside C (M or N <= 64: the 64-channel groups of the convolutions -- forward and data
  // gradient have N = 64, the weight gradient M = 64 --, attention heads) would only help with the staging.  Round 5: such a wave
  // JOINS the live quadrant beside it and takes the second k-step of every k-tile (the quadrant's owner keeps the first); the pair adds
  // its accumulators up through LDS behind the loop.  The 64-wide shapes are MFMA-bound in this kernel (a 3x3 convolution over 64
  // channels has 288 FLOP per HBM byte), so halving each live wave's MFMA chain is worth up to 2 x there.
  const bool m_narrow = p.M - m0 <= 64, n_narrow = p.N - n0 <= 64;           // uniform per workgroup
  const bool ksplit = m_narrow || n_narrow;
  int qm = wm, qn = wn, my_ks = 0;
  bool helper_idle = false;
  if (n_narrow && !m_narrow) { qn = 0; my_ks = wn; }
  else if (m_narrow && !n_narrow) { qm = 0; my_ks = wm; }
  else if (m_narrow && n_narrow) { qm = 0; qn = 0; my_ks = wave & 1; helper_idle = wave >= 2; }
  const bool quadrant_live = !helper_idle && m0 + qm * 64 < p.M && n0 + qn * 64 < p.N;
  constexpr bool WGRAD = AKS && BKS && OUTF32 && EPI == EPI_NONE;
  const bool row_sums = WGRAD && p.rsum_out != nullptr && bn == 0 && qn == 0;      // uniform per wave
  f32x4 racc[4];
  bf16x8 ones;
#pragma unroll
  for (int i = 0; i < 4; ++i) racc[i] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int i = 0; i < 8; ++i) ones[i] = f2bf(1.0f);
  if (row3) {
    char* const A3 = smem;
    char* const B2 = smem + 2 * A3_BYTES;
    // LDS row j of image gy <- tensor row m0 + j - 1 + a_view (gy - 1) pw (rows before the tensor wrap out of range: zeros), chunk
    // position XOR (j & 7) as frag_kc reads it; 4 issues of 32 rows by all waves + 8 rows by wave 0
    auto stage_a3 = [&](int gy, int b3) {
      char* const s3 = A3 + b3 * A3_BYTES;
      const int shift = p.a_view * (gy - 1) * p.pw - 1;
#pragma unroll
      for (int issue = 0; issue < 4; ++issue) {
        const int j = issue * 32 + (tid >> 3);
        const uint32_t off = (uint32_t)(((xa + j + shift) * p.lda + (((tid & 7) ^ (j & 7)) * 8)) * 2);
        __builtin_amdgcn_raw_ptr_buffer_load_lds(rsA, IA_LDS(s3 + issue * 4096 + wave * 1024), 16, off, 0, 0, 0);
      }
      if (wave == 0) {
        const int j = 128 + (lane >> 3);
        const uint32_t off = (uint32_t)(((xa + j + shift) * p.lda + (((lane & 7) ^ (j & 7)) * 8)) * 2);
        __builtin_amdgcn_raw_ptr_buffer_load_lds(rsA, IA_LDS(s3 + 16384), 16, off, 0, 0, 0);
      }
    };
    stage_a3(0, 0);
    stage_tile<BKS>(rsB, B2, 0, xb, p.ldb, p.K, tid, wave, b_org, p.b_view, p.pw, p.lcbk, p.lcbn);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    for (int kt = 0; kt < 9; ++kt) {
      const int gy = kt / 3, dxi = kt - 3 * gy, bb = kt & 1;
      if (kt + 1 < 9) stage_tile<BKS>(rsB, B2 + (bb ^ 1) * TILE_BYTES, kt + 1, xb, p.ldb, p.K, tid, wave, b_org, p.b_view, p.pw, p.lcbk, p.lcbn);
      if (dxi == 0 && gy < 2) stage_a3(gy + 1, (gy + 1) & 1);
      const char* sA = A3 + (gy & 1) * A3_BYTES;
      const char* sB = B2 + bb * TILE_BYTES;
      const int rowoff = 1 + p.a_view * (dxi - 1);
      if (quadrant_live)
#pragma unroll
      for (int ks = 0; ks < 2; ++ks) {
        if (ksplit && ks != my_ks) continue;
        bf16x8 af[4], bfr[4];
#pragma unroll
        for (int mi = 0; mi < 4; ++mi) af[mi] = frag_kc(sA, qm * 64 + mi * 16 + li + rowoff, ks * 4 + g);
#pragma unroll
        for (int ni = 0; ni < 4; ++ni) {
          if (!BKS) bfr[ni] = frag_kc(sB, qn * 64 + (li >> 2) * 16 + ni * 4 + (li & 3), ks * 4 + g);
          else      bfr[ni] = frag_ks(sB, ks * 32 + g * 8 + (li >> 2), qn * 64 + ni * 16 + (li & 3) * 4);
        }
        if (BKS) {
          asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
          __builtin_amdgcn_sched_barrier(0);
        }
#pragma unroll
        for (int mi = 0; mi < 4; ++mi)
#pragma unroll
          for (int ni = 0; ni < 4; ++ni)
            acc[mi][ni] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(bfr[ni], af[mi], acc[mi][ni], 0, 0, 0);
      }
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      __syncthreads();
    }
  } else
  for (int kt = kt0; kt < nk; ++kt) {
    const int buf = (kt - kt0) & 1;
    if (kt + 1 < nk) {
      char* nb = smem + (buf ^ 1) * 2 * TILE_BYTES;
      stage_tile<AKS>(rsA, nb, kt + 1, xa, p.lda, p.K, tid, wave, a_org, p.a_view, p.pw, p.lca, 0);
      stage_tile<BKS>(rsB, nb + TILE_BYTES, kt + 1, xb, p.ldb, p.K, tid, wave, b_org, p.b_view, p.pw, p.lcbk, p.lcbn);
    }
    const char* sA = smem + buf * 2 * TILE_BYTES;
    const char* sB = sA + TILE_BYTES;
    if (quadrant_live)
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      if (ksplit && ks != my_ks) continue;
      bf16x8 af[4], bfr[4];
#pragma unroll
      for (int mi = 0; mi < 4; ++mi) {
        if (!AKS) af[mi] = frag_kc(sA, qm * 64 + mi * 16 + li, ks * 4 + g);
        else      af[mi] = frag_ks(sA, ks * 32 + g * 8 + (li >> 2), qm * 64 + mi * 16 + (li & 3) * 4);
      }
#pragma unroll
      for (int ni = 0; ni < 4; ++ni) {
        // k-contiguous B: fragment row i <-> n = (i>>2)*16 + ni*4 + (i&3), so lane group g ends up
        // holding 16 consecutive n; k-strided B: plain n = ni*16 + i (conflict-free transpose read).
        if (!BKS) bfr[ni] = frag_kc(sB, qn * 64 + (li >> 2) * 16 + ni * 4 + (li & 3), ks * 4 + g);
        else      bfr[ni] = frag_ks(sB, ks * 32 + g * 8 + (li >> 2), qn * 64 + ni * 16 + (li & 3) * 4);
      }
      if (AKS || BKS) {   // the transpose reads are asm (common.h): order the MFMAs behind their data
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_sched_barrier(0);
      }
#pragma unroll
      for (int mi = 0; mi < 4; ++mi)
#pragma unroll
        for (int ni = 0; ni < 4; ++ni)
          acc[mi][ni] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(bfr[ni], af[mi], acc[mi][ni], 0, 0, 0);
      if (WGRAD && row_sums)          // D[n][m] = sum_k 1 * A[m][k] for every n: each lane's column li holds the sum of its m
#pragma unroll
        for (int mi = 0; mi < 4; ++mi) racc[mi] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ones, af[mi], racc[mi], 0, 0, 0);
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
  }

  if (ksplit) {
    // the helper (k-step 1) hands its sums to the quadrant's owner: 20 x 16-byte columns per lane, lane-major inside a column so
    // that both sides move whole 1-KiB lines; the k-tile buffers are free behind the loop's last barrier
    float* const xch = reinterpret_cast<float*>(smem) + (size_t)(qm * 2 + qn) * (20 * 64 * 4);
    if (quadrant_live && my_ks == 1) {
#pragma unroll
      for (int mi = 0; mi < 4; ++mi) {
#pragma unroll
        for (int ni = 0; ni < 4; ++ni) *reinterpret_cast<f32x4*>(xch + ((mi * 4 + ni) * 64 + lane) * 4) = acc[mi][ni];
        *reinterpret_cast<f32x4*>(xch + ((16 + mi) * 64 + lane) * 4) = racc[mi];
      }
    }
    __syncthreads();
    if (!quadrant_live || my_ks == 1) return;
#pragma unroll
    for (int mi = 0; mi < 4; ++mi) {
#pragma unroll
      for (int ni = 0; ni < 4; ++ni) acc[mi][ni] += *reinterpret_cast<const f32x4*>(xch + ((mi * 4 + ni) * 64 + lane) * 4);
      racc[mi] += *reinterpret_cast<const f32x4*>(xch + ((16 + mi) * 64 + lane) * 4);
    }
  }

#pragma unroll
  for (int mi = 0; mi < 4; ++mi) {
    const int m = m0 + qm * 64 + mi * 16 + li;
    if (m >= p.M) continue;
#pragma unroll
    for (int ni = 0; ni < 4; ++ni) {
      const int n = n0 + qn * 64 + (BKS ? ni * 16 + g * 4 : g * 16 + ni * 4);
      if (n >= p.N) continue;
      epi_store4<EPI, OUTF32>(p, m, n, acc[mi][ni]);
    }
  }
  if (WGRAD && row_sums && g == 0) {
#pragma unroll
    for (int mi = 0; mi < 4; ++mi) {
      const int m = m0 + qm * 64 + mi * 16 + li;
      if (m >= p.M) continue;
      if (p.splits > 1) p.rsum_ws[((size_t)grp * p.splits + p.split_id) * p.M + m] = racc[mi][0];
      else p.rsum_out[(size_t)grp * p.M + m] += racc[mi][0];
    }
  }
}
}  // namespace t128

// ============================================================================== T256W (4 waves, 128 x 128 per wave, 32x32x16)
// 256 x 256 x 64 block tile per 256-thread workgroup, ONE wave per SIMD owning a 128 x 128 part (256 accumulators in AGPRs): 8 fragment
// reads per 16 MFMAs, i.e. 128 + 64 KiB of LDS traffic per k-tile -- the 64 x 64 wave tile of T128 saturates the LDS port.  (Until
// round 4 a second 256 x 256 kernel, T256, ran two waves per SIMD on 128 x 64 wave tiles -- 12 reads per 16 MFMAs, 192 + 64 KiB -- for
// the VALU-heavy epilogues; removed once this kernel won those too: bias + GELU 412 -> 405 us, x GELU' + column sums 317 -> 313 us at
// 32640 x 4096 x 1024, step +0.65 % on the same box.)
// The workgroup is persistent over output tiles (one workgroup per CU: the kernel takes all of its LDS): the DMA of the NEXT tile's
// first two k-tiles is issued before the current tile's epilogue, which stages through LDS outside the k-tile buffers, so the ~2 us
// HBM round trip of a tile prologue hides behind the epilogue instead of idling the CU.
// With one wave per SIMD nothing else hides latency, so the wave pipelines itself, on the schedule of
// the library's hand-written 256x256x64 kernels (read off their disassembly): the WHOLE k-tile of fragments lives in registers
// (four sets of 8 fragments), so the LDS buffer of k-tile u is free after the first HALF of iteration u; k-tile u+2 is then
// requested piece by piece between the MFMAs of the second half (one 1-KiB LDS-DMA per two MFMAs, never a burst), stays in flight
// for a whole iteration and is only waited for with a counted vmcnt(8) in front of the last k-step of iteration u+1, where the first
// fragments of k-tile u+1 are read.  Two workgroup barriers per k-tile, each behind issued MFMAs.
//   k-step 0: MFMAs on set 0 | fragment reads of sets 1 and 2 (one per MFMA)
//   k-step 1: MFMAs on set 1 | reads of set 3;  lgkmcnt(0), barrier B1: every wave holds all of k-tile u -> its buffer is free
//   k-step 2: MFMAs on set 2 | DMA pieces 0..7 of k-tile u+2
//   k-step 3: vmcnt(8), barrier B2: k-tile u+1 has landed;  MFMAs on set 3 | reads of set 0 of k-tile u+1, DMA pieces 8..15
// (the forward GEMMs run a second schedule, ROUND: see main_loop)
namespace t256w {
constexpr int BM = 256, BN = 256, TILE_BYTES = 32768;        // one operand's k-tile: 256 rows x 64 k (or 64 k x 256 columns) of bf16
constexpr int STAGE_BYTES = 16 * 64 * 4;                   // epilogue staging slot (16 rows x 64 columns fp32); each of the four waves owns two
// EPI_NONE_BLK: a k-slab's live-block mask is one 32-bit word per lane, two bits per k-tile -- 1024 k-tiles at the most.  The one statement
// of that limit (the host asks it in gemm_core and in ia_gemm_wgrad_rows_filters): a longer k-slab runs every row.
inline bool blk_mask_fits(int slab_ktiles) { return slab_ktiles <= 64 * 32 / 2; }
// EPI_NONE_STP: four bits per k-tile -- 512 k-tiles at the most; a longer k-slab takes the block walk
inline bool step_mask_fits(int slab_ktiles) { return slab_ktiles <= 64 * 32 / 4; }
constexpr uint32_t OOB_HALF = 0x80000000u;                 // behind every buffer window (< 2 GiB), and three piece advances on top do not wrap
constexpr int LDS_BYTES = 2 * 2 * TILE_BYTES + 8 * STAGE_BYTES;   // 128 KiB k-tile double buffer (A | B, twice) + 4 x 8 KiB = all 160 KiB of the CU

// One operand's four fragments of a k-step.  A k-strided operand's fragment arrives as two transpose reads: the halves are kept
// apart until the wait (the wait asm ties the RAW read destinations; assembling the 128-bit value earlier could be scheduled as
// register copies in front of the wait).
template <bool KS> struct Op;
template <> struct Op<false> { bf16x8 v[4]; };
template <> struct Op<true> { s16x4 lo[4], hi[4]; };
IA_DEV bf16x8 frag_of(const Op<false>& o, int j) { return o.v[j]; }
IA_DEV bf16x8 frag_of(const Op<true>& o, int j) {
  s16x8 r = {o.lo[j][0], o.lo[j][1], o.lo[j][2], o.lo[j][3], o.hi[j][0], o.hi[j][1], o.hi[j][2], o.hi[j][3]};
  return __builtin_bit_cast(bf16x8, r);
}

template <int IMM>
IA_DEV bf16x8 rd128(uint32_t addr) {
  bf16x8 d;
  asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(d) : "v"(addr), "n"(IMM));
  return d;
}
template <int IMM>
IA_DEV s16x4 rd_tr(uint32_t addr) {
  s16x4 d;
  asm volatile("ds_read_b64_tr_b16 %0, %1 offset:%2" : "=v"(d) : "v"(addr), "n"(IMM));
  return d;
}

// Per-lane LDS byte offsets of one operand's fragments inside a k-tile buffer.  k-contiguous tile ([256 rows][64 k], chunk XOR
// (row>>1)&7): fragment (j, ks) of rows x0 + j*32 + li sits at base[ks] + j*4096 -- the XOR only depends on the lane and ks.
// k-strided tile ([64 k][256 x], 32-byte slot XOR (k&3)<<2): fragment (j, ks) of columns x0 + j*32.. sits at base[j] + ks*8192 --
// the XOR lands on the bits j occupies, so it is folded per j.  (x0 = 0 or 128: the wave's half of the tile.)
template <bool KS>
IA_DEV void frag_bases(uint32_t (&base)[4], uint32_t tile_addr, int x0, int lane, int nperm_row) {
  if (!KS) {
    const int hh = lane >> 5;
    const int row = x0 + nperm_row;                       // li, or the permuted row of a k-contiguous B operand
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) base[ks] = tile_addr + row * 128 + ((((ks * 2 + hh) ^ ((row >> 1) & 7))) << 4);
  } else {
    const int p = lane & 15, G = lane >> 4;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int row = 8 * (G >> 1) + (p >> 2);            // + ks*16 through the immediate
      const int col = x0 + j * 32 + 16 * (G & 1) + (p & 3) * 4;
      base[j] = tile_addr + row * 512 + ((((col >> 3) ^ ((row & 3) << 2))) << 4) + (col & 7) * 2;
    }
  }
}

// wait until at most N LDS operations are outstanding and tie the read destinations to the wait (the MFMAs that consume them
// cannot be scheduled above it)
template <int N> IA_DEV void tie(Op<false>& o) {
  asm volatile("s_waitcnt lgkmcnt(%4)" : "+v"(o.v[0]), "+v"(o.v[1]), "+v"(o.v[2]), "+v"(o.v[3]) : "n"(N));
}
// several fragment sets behind ONE wait (k-contiguous sets: 4 registers each; six sets are 24 of the 30 operands an asm may have)
template <int N> IA_DEV void tie2(Op<false>& a, Op<false>& b) {
  asm volatile("s_waitcnt lgkmcnt(%8)" : "+v"(a.v[0]), "+v"(a.v[1]), "+v"(a.v[2]), "+v"(a.v[3]), "+v"(b.v[0]), "+v"(b.v[1]), "+v"(b.v[2]), "+v"(b.v[3]) : "n"(N));
}
template <int N> IA_DEV void tie6(Op<false>& a, Op<false>& b, Op<false>& c, Op<false>& d, Op<false>& e, Op<false>& f) {
  asm volatile("s_waitcnt lgkmcnt(%24)"
               : "+v"(a.v[0]), "+v"(a.v[1]), "+v"(a.v[2]), "+v"(a.v[3]), "+v"(b.v[0]), "+v"(b.v[1]), "+v"(b.v[2]), "+v"(b.v[3]),
                 "+v"(c.v[0]), "+v"(c.v[1]), "+v"(c.v[2]), "+v"(c.v[3]), "+v"(d.v[0]), "+v"(d.v[1]), "+v"(d.v[2]), "+v"(d.v[3]),
                 "+v"(e.v[0]), "+v"(e.v[1]), "+v"(e.v[2]), "+v"(e.v[3]), "+v"(f.v[0]), "+v"(f.v[1]), "+v"(f.v[2]), "+v"(f.v[3])
               : "n"(N));
}
template <int N> IA_DEV void tie(Op<true>& o) {
  asm volatile("s_waitcnt lgkmcnt(%8)" : "+v"(o.lo[0]), "+v"(o.lo[1]), "+v"(o.lo[2]), "+v"(o.lo[3]), "+v"(o.hi[0]), "+v"(o.hi[1]), "+v"(o.hi[2]), "+v"(o.hi[3]) : "n"(N));
}
template <int N> IA_DEV void tie2(Op<true>& a, Op<true>& b) { tie<N>(a); tie<N>(b); }
template <int N> IA_DEV void tie6(Op<true>& a, Op<true>& b, Op<true>& c, Op<true>& d, Op<true>& e, Op<true>& f) {
  tie<N>(a); tie<N>(b); tie<N>(c); tie<N>(d); tie<N>(e); tie<N>(f);
}


// fragment j (0..3: A, 4..7: B) of k-step S of the k-tile at bufoff
template <int S, bool KS>
IA_DEV void read_frag(Op<KS>& f, int j, const uint32_t (&base)[4], uint32_t bufoff) {
  if constexpr (!KS) {
    const uint32_t a = base[S] + bufoff;
    if (j == 0) f.v[0] = rd128<0>(a);
    if (j == 1) f.v[1] = rd128<4096>(a);
    if (j == 2) f.v[2] = rd128<8192>(a);
    if (j == 3) f.v[3] = rd128<12288>(a);
  } else {
    f.lo[j] = rd_tr<S * 8192>(base[j] + bufoff);
    f.hi[j] = rd_tr<S * 8192 + 4 * 512>(base[j] + bufoff);
  }
}

// the 16 MFMAs of one k-step on the fragment sets fa / fb; filler(i) is issued right behind MFMA i and pinned there
// FRESH (the first k-step of a tile's peeled first trip): the MFMAs take a zero C operand, so nothing has to clear the accumulators
// (two 16x16x32 MFMAs in place of each 32x32x16 ran 8-14 % slower: the MFMA shape is not what separates this loop from the vendor's)
// PIN (the walk forms, whose fillers are long runs of scalar arithmetic): each MFMA's result passes through an empty volatile asm in
// front of its filler -- an MFMA has no side effect, and instruction selection is otherwise free to emit it behind fillers that have
// one (with the walk in the gaps the first MFMA of the trip came out behind 114 instructions).  The other forms are not touched.
template <bool FRESH, bool PIN = false, typename FA, typename FB, typename Filler>
IA_DEV void mfma_step(f32x16 (&acc)[4][4], const FA& fa, const FB& fb, Filler&& filler) {
  bf16x8 va[4], vb[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) { va[j] = frag_of(fa, j); vb[j] = frag_of(fb, j); }
#pragma unroll
  for (int mi = 0; mi < 4; ++mi)
#pragma unroll
    for (int ni = 0; ni < 4; ++ni) {
      if constexpr (FRESH) {
        const f32x16 z = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        acc[mi][ni] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(vb[ni], va[mi], z, 0, 0, 0);
      } else acc[mi][ni] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(vb[ni], va[mi], acc[mi][ni], 0, 0, 0);
      if constexpr (PIN) asm volatile("" : "+a"(acc[mi][ni]));
      filler(mi * 4 + ni);
      __builtin_amdgcn_sched_barrier(0);
    }
}

// EPI_ROWS: the eight 32-row blocks of remapped M-tile bm (-1: the list has no such entry -- the tail of the last tile).  One scalar
// load, waited for on the spot (lgkmcnt(0) is the strictest form of every LDS wait around it); the address is uniform and 32-byte
// aligned (eight header words in front of the list, eight entries per tile).
struct Blk8 { int b[8]; };
struct RowOff { uint32_t o[8]; };      // byte offset of each A piece's first row (the scalar offset of its DMA)
struct RowBlk { int r[4]; };           // first row of each of the wave's four 32-row blocks, -1 = none
constexpr int ROW_BLK_HDR = 8;         // list header: [0] live blocks, [1] dead blocks, [2] blocks; the live list follows
IA_DEV Blk8 load_blk8(const int* list, int bm, int n_live) {
  typedef int i32x8 __attribute__((ext_vector_type(8)));
  const uint64_t a64 = (uint64_t)(list + ROW_BLK_HDR + bm * 8);
  const uint32_t alo = __builtin_amdgcn_readfirstlane((uint32_t)a64), ahi = __builtin_amdgcn_readfirstlane((uint32_t)(a64 >> 32));
  const uint64_t addr = ((uint64_t)ahi << 32) | alo;
  i32x8 v;
  asm volatile("s_nop 4\n\ts_load_dwordx8 %0, %1, 0x0\n\ts_waitcnt lgkmcnt(0)" : "=&s"(v) : "s"(addr) : "memory");
  Blk8 r;
#pragma unroll
  for (int j = 0; j < 8; ++j) r.b[j] = bm * 8 + j < n_live ? v[j] : -1;
  return r;
}

// GemmArgs::rows_guarded (EPI_ROWS + EPI_BIAS only): the launch is ONE M-tile made of the live blocks behind the last whole 128-row part
// of M -- at most four, the last entries of the ascending live list, taken from its end backwards (so the ones that exist come first;
// the kernel runs no tile when the first does not exist, so b[0], which stands in for the missing ones, is always a real block).
template <bool GUARDABLE>
IA_DEV Blk8 tile_blocks(const GemmArgs& p, int bm, int n_live) {
  if constexpr (GUARDABLE) {
    if (p.rows_guarded) {
      const int tb0 = (p.M & ~127) >> 5;
      Blk8 r;
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        int v = -1;
        if (j < 4 && n_live - 1 - j >= 0) v = __builtin_amdgcn_readfirstlane(p.row_blk[ROW_BLK_HDR + n_live - 1 - j]);
        r.b[j] = v >= tb0 ? v : -1;
      }
      return r;
    }
  }
  return load_blk8(p.row_blk, bm, n_live);
}

// EPI_SLABS: the list ia_row_slabs wrote -- the header of ia_row_blocks (counted in slabs), then 32 entries per M-tile in the order
// [wave][piece]: entry w * 8 + j of a tile is its slab 4j + w in ascending order, the 8 rows wave w carries of DMA piece j.  The entries
// behind the last live slab of the last tile are -1.  A wave's eight DMA sources are one aligned 32-byte scalar load, its sixteen
// epilogue rows (pieces 4 wm .. 4 wm + 3 of every wave's run) four 16-byte ones.
constexpr int SLAB_TILE = 32;
struct RowSlab { int r[16]; };         // first row of the slab behind pass it of the wave's block mi at [mi * 4 + it], negative = none
IA_DEV int slab_pos(int t) { return (t & 3) * 8 + (t >> 2); }      // where slab t of a tile sits among its 32 entries
IA_DEV const int* uniform_ptr(const int* q) {
  const uint64_t a64 = (uint64_t)q;
  const uint32_t alo = __builtin_amdgcn_readfirstlane((uint32_t)a64), ahi = __builtin_amdgcn_readfirstlane((uint32_t)(a64 >> 32));
  return (const int*)(((uint64_t)ahi << 32) | alo);
}
// GemmArgs::rows_guarded in slabs: slab t of the ONE M-tile is the t-th live slab from the end of the list, as long as it lies behind the
// last whole 128-row part of M (at most sixteen do); -1 behind them.
IA_DEV int guarded_slab(const GemmArgs& p, int t, int n_live) {
  const int g = n_live - 1 - t;
  if (t >= 16 || g < 0) return -1;
  const int v = __builtin_amdgcn_readfirstlane(p.row_blk[ROW_BLK_HDR + (g & ~31) + slab_pos(g & 31)]);
  return v * 8 >= (p.M & ~127) ? v : -1;
}
// the byte offsets of the eight A pieces of wave `wave` (a slab the tile does not have: the tensor's first rows, computed and never stored)
template <bool GUARDABLE>
IA_DEV RowOff slab_offsets(const GemmArgs& p, int bm, int wave, int n_live) {
  typedef int i32x8 __attribute__((ext_vector_type(8)));
  RowOff ro;
  if constexpr (GUARDABLE) {
    if (p.rows_guarded) {
#pragma unroll
      for (int j = 0; j < 8; ++j) { const int v = guarded_slab(p, j * 4 + wave, n_live); ro.o[j] = (uint32_t)(v >= 0 ? v : 0) * (uint32_t)(8 * p.lda * 2); }
      return ro;
    }
  }
  const int* const addr = uniform_ptr(p.row_blk + ROW_BLK_HDR + bm * SLAB_TILE + wave * 8);
  i32x8 v;
  asm volatile("s_nop 4\n\ts_load_dwordx8 %0, %1, 0x0\n\ts_waitcnt lgkmcnt(0)" : "=&s"(v) : "s"(addr) : "memory");
#pragma unroll
  for (int j = 0; j < 8; ++j) ro.o[j] = (uint32_t)(v[j] >= 0 ? v[j] : 0) * (uint32_t)(8 * p.lda * 2);
  return ro;
}
// the sixteen epilogue rows of a wave of wave-row wm
template <bool GUARDABLE>
IA_DEV RowSlab slab_rows(const GemmArgs& p, int bm, int wm, int n_live) {
  typedef int i32x4 __attribute__((ext_vector_type(4)));
  RowSlab rs;
  if constexpr (GUARDABLE) {
    if (p.rows_guarded) {
#pragma unroll
      for (int c = 0; c < 16; ++c) rs.r[c] = guarded_slab(p, (wm * 4 + (c >> 2)) * 4 + (c & 3), n_live) * 8;
      return rs;
    }
  }
  const int* const addr = uniform_ptr(p.row_blk + ROW_BLK_HDR + bm * SLAB_TILE + wm * 4);
  i32x4 v0, v1, v2, v3;
  asm volatile("s_nop 4\n\ts_load_dwordx4 %0, %4, 0x0\n\ts_load_dwordx4 %1, %4, 0x20\n\ts_load_dwordx4 %2, %4, 0x40\n\ts_load_dwordx4 %3, %4, 0x60\n\t"
               "s_waitcnt lgkmcnt(0)" : "=&s"(v0), "=&s"(v1), "=&s"(v2), "=&s"(v3) : "s"(addr) : "memory");
#pragma unroll
  for (int mi = 0; mi < 4; ++mi) { rs.r[mi * 4] = v0[mi] * 8; rs.r[mi * 4 + 1] = v1[mi] * 8; rs.r[mi * 4 + 2] = v2[mi] * 8; rs.r[mi * 4 + 3] = v3[mi] * 8; }
  return rs;
}

// Walk over the set bits of a k-slab's live-block mask (one bit per 32-row block) in increasing order.  Lane l of `mv` holds bits
// 32l .. 32l+31 of the slab (every wave holds the same 64 words, fetched once in front of the first prologue DMA); the walk itself is SALU
// plus one v_readlane per step -- no memory operation, so it can sit next to the k loop's counted waits, and no branch.  Once the bits
// are used up next() keeps returning the index behind the last one it gave: a look-ahead piece past the end then addresses the block
// right behind the last one consumed, as the dense kernel's does, where main_loop does not send it out of range.
struct LiveWalk {
  uint64_t rest;      // words with a set bit that have not been opened yet
  uint32_t w;         // bits of the open word not handed out yet
  int wi, cur;        // the open word; the last index handed out
};
IA_DEV void live_start(LiveWalk& k, uint32_t mv) { k.rest = __ballot(mv != 0u); k.w = 0u; k.wi = 0; k.cur = -1; }
// One step in two halves, so that the k loop can give each a MFMA gap of its own: live_open opens the next word with a set bit when the
// open one is used up, live_take hands out the open word's lowest bit.
IA_DEV void live_open(LiveWalk& k, uint32_t mv) {
  const bool open = k.w == 0u, any = k.rest != 0ull;
  const int wi = open ? (any ? __builtin_ctzll(k.rest) : 0) : k.wi;
  const uint32_t fetched = __builtin_amdgcn_readlane(mv, wi);
  k.w = open ? (any ? fetched : 0u) : k.w;
  k.rest = open ? (k.rest & (k.rest - 1ull)) : k.rest;
  k.wi = wi;
}
IA_DEV int live_take(LiveWalk& k) {
  const uint32_t w = k.w;
  const int bit = __builtin_ctz(w | 0x80000000u);      // (w == 0: unused)
  const int idx = w != 0u ? k.wi * 32 + bit : k.cur + 1;
  // (the lowest set bit cleared by its index: `w & (w - 1)` next to `w == 0` becomes a subtract-with-borrow on the VALU)
  k.w = w & ~(1u << bit) & (w != 0u ? 0xFFFFFFFFu : 0u); k.cur = idx;
  return idx;
}
IA_DEV int live_next(LiveWalk& k, uint32_t mv) { live_open(k, mv); return live_take(k); }

// BLK (EPI_NONE_BLK; both operands k-strided): the k loop runs over the n_blk set bits of live_mv (the slab's live 32-row blocks, see
// LiveWalk) instead of k-tiles 0 .. n_tiles-1 of the slab -- two blocks per trip (n_tiles = ceil(n_blk / 2)); the upper half of the
// last trip of an odd count goes out of range and arrives as zeros.
// ROWS (k-contiguous A): piece j of A starts at row offset ro.o[j] (a scalar, where j * stepA sits otherwise) of a window over all of A.
// SLAB: ro.o[j] is this WAVE's slab of piece j -- the lane offset keeps the row inside the slab (row & 7) and the swizzle of the LDS row.
template <bool AKS, bool BKS, int PEND, bool PEEL_OK = true, bool BLK = false, bool ROWS = false, bool SLAB = false, bool STP = false>
IA_DEV void main_loop(const GemmArgs& p, char* smem, f32x16 (&acc)[4][4], __amdgpu_buffer_rsrc_t rsA, __amdgpu_buffer_rsrc_t rsB, int xa, int xb,
                      int kt0, int ktaA0, int ktaB0, int n_tiles, int nk_all, int wm, int wn, int wave, int lane, bool prologue_only,
                      bool stores_in_flight, uint32_t live_mv = 0u, RowOff ro = RowOff{}, int n_blk = 0) {
  static_assert(!ROWS || !AKS, "the row remap moves the pieces of a k-contiguous A");
  static_assert(!BLK || (AKS && BKS), "the live-block walk sets the running lane offsets of two k-strided operands");
  static_assert(!STP || BLK, "the 16-row step walk is a form of the live-block walk");
  // BLK: a trip's k-tile is made of NQ parts of the walk (two 32-row blocks, or STP: four 16-row steps), PP DMA pieces of 8 k rows each
  constexpr int NQ = STP ? 4 : 2, PP = 8 / NQ, QSH = STP ? 2 : 1;
  constexpr bool ROUND = !AKS && !BKS;      // the k loop's schedule (below)
  const int li = lane & 31;
  const int gt = wave * 64 + lane;                  // thread index inside the workgroup (0..255)
  // ---- DMA: 8 pieces per operand and k-tile.  One per-lane byte offset serves all 8 pieces of an operand: the swizzled chunk a lane
  // fetches does not depend on the piece (the row advance per piece is a multiple of the swizzle period), so the piece and k-tile
  // advances are both scalars folded into the instruction's soffset.
  uint32_t voffA, stepA, voffB, stepB;
  if (!AKS) { const int row = gt >> 3; voffA = (uint32_t)(((xa + (SLAB ? row & 7 : row)) * p.lda + (((gt & 7) ^ ((row >> 1) & 7)) * 8)) * 2); stepA = (uint32_t)(32 * p.lda * 2); }
  else { const int row = gt >> 5; voffA = (uint32_t)((row * p.lda + xa + (((gt & 31) ^ ((row & 3) << 2)) * 8)) * 2); stepA = (uint32_t)(8 * p.lda * 2); }
  if (!BKS) { const int row = gt >> 3; voffB = (uint32_t)(((xb + row) * p.ldb + (((gt & 7) ^ ((row >> 1) & 7)) * 8)) * 2); stepB = (uint32_t)(32 * p.ldb * 2); }
  else { const int row = gt >> 5; voffB = (uint32_t)((row * p.ldb + xb + (((gt & 31) ^ ((row & 3) << 2)) * 8)) * 2); stepB = (uint32_t)(8 * p.ldb * 2); }
  const uint32_t kstepA = AKS ? (uint32_t)(BK * p.lda * 2) : (uint32_t)(BK * 2), kstepB = BKS ? (uint32_t)(BK * p.ldb * 2) : (uint32_t)(BK * 2);
  // the k index of this lane's 16 bytes inside a k-tile: k-strided piece j holds k rows j*8 + (gt>>5), a k-contiguous piece the chunk
  const int klA = AKS ? (gt >> 5) : ((gt & 7) ^ (((gt >> 3) >> 1) & 7)) * 8;
  const int klB = BKS ? (gt >> 5) : ((gt & 7) ^ (((gt >> 3) >> 1) & 7)) * 8;
  char* const my_part = smem + wave * 1024;
  const int dbg = IA_GEMM_DBG_HOOKS ? p.dbg : 0;       // the timing ablations (IA_GEMM_DBG bits 2 / 4 / 16) exist in tools builds only
  const bool dma_on = !(dbg & 2);
  // BLK: the slab-relative indices of the first 2 NQ live parts (the prologue's two k-tiles, part by part)
  [[maybe_unused]] LiveWalk lw;
  [[maybe_unused]] int live01[2][NQ] = {};
  if constexpr (BLK) {
    live_start(lw, live_mv);
#pragma unroll
    for (int t = 0; t < 2 * NQ; ++t) live01[t / NQ][t % NQ] = live_next(lw, live_mv);
  }

  // piece i (0..7: A, 8..15: B) of k-tile u -> buffer u & 1.  Branch-free (a branch next to the accumulator updates makes hipcc copy
  // all 256 of them): lim = number of valid k in this k-tile (0 for a k-tile past the end: the whole piece goes out of range and
  // writes zeros into a buffer nobody reads any more); the address advance per piece and k-tile is a scalar (soffset).
  auto dma_piece = [&](int u, int i) {
    const bool isB = i >= 8;
    const int j = i & 7;
    char* dst = my_part + (isB ? TILE_BYTES : 0) + (u & 1) * 2 * TILE_BYTES + j * 4096;
    if constexpr (BLK) {
      // pieces 0 .. 3: rows 0 .. 31 of the lower half's block, pieces 4 .. 7 of the upper half's (STP: pieces 2q and 2q + 1 are the 16 rows
      // of the trip's step q); a part the slab has no block / step for goes out of range (zeros).  The whole row address sits in the
      // lane offset: the partial last block / step of K ends at the window's end.
      const int h = j / PP;
      const int b = live01[u & 1][h];
      const uint32_t soff = (uint32_t)b * ((isB ? kstepB : kstepA) >> QSH) + (uint32_t)(j % PP) * (isB ? stepB : stepA);
      const uint32_t off = (dma_on && NQ * u + h < n_blk) ? (isB ? voffB : voffA) + soff : OOB;
      __builtin_amdgcn_raw_ptr_buffer_load_lds(isB ? rsB : rsA, IA_LDS(dst), 16, off, 0, 0, 0);
      return;
    }
    const int kt = kt0 + u;
    const int kta = (dbg & 4) ? 0 : (isB ? ktaB0 : ktaA0) + u;      // dbg 4: every k-tile re-fetches k-tile 0 (cache-resident)
    const bool ks = isB ? BKS : AKS;
    const uint32_t soff = (uint32_t)kta * (isB ? kstepB : kstepA) + ((ROWS && !isB) ? ro.o[j] : (uint32_t)j * (isB ? stepB : stepA));
    if (ks) {
      // k-strided operand: k is the ROW of the tensor, so a piece past K (the tail of the last k-tile, the look-ahead k-tiles behind it)
      // lies behind the end of the buffer window -- provided its whole address sits in the LANE offset (the hardware's range check does
      // not see the scalar offset): one v_add per piece instead of add + compare + select.  (A split-K slab's look-ahead reads the next
      // slab's first rows instead of zeros: nobody consumes that buffer.)  Data gradient +4 %, weight gradient +0.7 %; the memory-side
      // fetches of both went UP 4-8 % with it (FETCH_SIZE 0.996 -> 1.076 GB per weight-gradient launch, same box, against compare +
      // select per piece): far more than the two look-ahead k-tiles -- the workgroups that share a panel out of one L2 drift further apart.
      const uint32_t off = dma_on ? (isB ? voffB : voffA) + soff : OOB;
      __builtin_amdgcn_raw_ptr_buffer_load_lds(isB ? rsB : rsA, IA_LDS(dst), 16, off, 0, 0, 0);
    } else {
      const int lim = (u < n_tiles && dma_on) ? p.K - kt * BK : 0;
      const uint32_t off = (isB ? klB : klA) + (ks ? j * 8 : 0) < lim ? (isB ? voffB : voffA) : OOB;
      __builtin_amdgcn_raw_ptr_buffer_load_lds(isB ? rsB : rsA, IA_LDS(dst), 16, off, (int)soff, 0, 0);
    }
  };

  // ROUND schedule (k-contiguous operands): the lane offset of a k-tile's pieces is the same for all eight pieces of an operand -- whole
  // k-tile, K tail, or out of range past the last k-tile -- and is formed where the schedule has room, not at the first piece
  auto off_of = [&](int u, bool isB) -> uint32_t {
    const int lim = (u < n_tiles && dma_on) ? p.K - (kt0 + u) * BK : 0;
    return (isB ? klB : klA) < lim ? (isB ? voffB : voffA) : OOB;
  };
  auto dma_c = [&](int u, int i, uint32_t off) {
    const bool isB = i >= 8;
    const int j = i & 7;
    char* dst = my_part + (isB ? TILE_BYTES : 0) + (u & 1) * 2 * TILE_BYTES + j * 4096;
    const int kta = (dbg & 4) ? 0 : (isB ? ktaB0 : ktaA0) + u;
    const uint32_t soff = (uint32_t)kta * (isB ? kstepB : kstepA) + ((ROWS && !isB) ? ro.o[j] : (uint32_t)j * (isB ? stepB : stepA));
    __builtin_amdgcn_raw_ptr_buffer_load_lds(isB ? rsB : rsA, IA_LDS(dst), 16, off, (int)soff, 0, 0);
  };

  // second schedule (a k-strided operand): in-loop pieces of k-tile u+2; the k-strided operand's k-tile advance lives in a running lane offset
  uint32_t runA = voffA + (uint32_t)((dbg & 4) ? 0 : ktaA0 + 2) * kstepA, runB = voffB + (uint32_t)((dbg & 4) ? 0 : ktaB0 + 2) * kstepB;
  // BLK: NQ running lane offsets per operand, one per part of the trip's k-tile.  They are set under k-step 1 of the trip whose
  // k-steps 2 and 3 send them out (walk_open, walk_take, walk_offsets): nothing of the walk stands in front of the trip's first MFMA or behind its last.
  [[maybe_unused]] uint32_t runQA[NQ] = {}, runQB[NQ] = {};
  [[maybe_unused]] int nextQ[NQ] = {};           // the parts' indices of the walk between walk_take and walk_offsets
  auto dma_run = [&](int u, int i) {
    const bool isB = i >= 8;
    if (!(isB ? BKS : AKS) || (dbg & 4)) { dma_piece(u, i); return; }
    const int j = i & 7;
    char* dst = my_part + (isB ? TILE_BYTES : 0) + (u & 1) * 2 * TILE_BYTES + j * 4096;
    if constexpr (BLK) {
      const uint32_t off = (isB ? runQB[j / PP] : runQA[j / PP]) + (uint32_t)(j % PP) * (isB ? stepB : stepA);
      __builtin_amdgcn_raw_ptr_buffer_load_lds(isB ? rsB : rsA, IA_LDS(dst), 16, dma_on ? off : OOB, 0, 0, 0);
      return;
    }
    const uint32_t off = (isB ? runB : runA) + (uint32_t)j * (isB ? stepB : stepA);
    __builtin_amdgcn_raw_ptr_buffer_load_lds(isB ? rsB : rsA, IA_LDS(dst), 16, dma_on ? off : OOB, 0, 0, 0);
  };

  if (prologue_only) {       // called ahead of time (before the previous tile's epilogue): just start the first two k-tiles
#pragma unroll
    for (int i = 0; i < 16; ++i) dma_piece(0, i);
#pragma unroll
    for (int i = 0; i < (ROUND ? 12 : 16); ++i) dma_piece(1, i);      // (zero-filled when it does not exist; the rest: see the loops)
    return;
  }
  // the prologue DMA of this tile.  After a full-tile epilogue exactly PEND store instructions were issued behind it and
  // may stay in flight (vmcnt retires in order: at most PEND outstanding <=> every older DMA piece has landed).
  if (stores_in_flight) asm volatile("s_waitcnt vmcnt(%0)" : : "n"(PEND < 60 ? PEND : 60) : "memory");
  else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __builtin_amdgcn_s_barrier();

  // ---- fragment addresses
  const int nperm = ((li >> 2) & 1) * 16 + (li >> 3) * 4 + (li & 3);      // B row <-> n so that a lane ends up with 16 consecutive columns
  uint32_t baseA[4], baseB[4];
  const uint32_t smem_addr = ia_lds_addr(smem);
  frag_bases<AKS>(baseA, smem_addr, wm * 128, lane, li);
  frag_bases<BKS>(baseB, smem_addr + TILE_BYTES, wn * 128, lane, nperm);
  constexpr int NRA = AKS ? 8 : 4, NRB = BKS ? 8 : 4, NR = NRA + NRB;      // LDS operations of one fragment set
  constexpr int NR15 = NR > 15 ? 15 : NR;

  Op<AKS> a0, a1, a2, a3;
  Op<BKS> b0, b1, b2, b3;
#pragma unroll
  for (int j = 0; j < 4; ++j) read_frag<0>(a0, j, baseA, 0u);
#pragma unroll
  for (int j = 0; j < 4; ++j) read_frag<0>(b0, j, baseB, 0u);

  using Acc = std::false_type;

  uint32_t bo = 0;
  int u = 0;
  // Two schedules.  ROUND (both operands k-contiguous: the forward GEMMs): every fragment of k-tile u is requested under k-step 0 (24 / 36
  // LDS reads behind 12 MFMAs), the buffer is handed back after a QUARTER of the k-tile, and the 16 DMA pieces of a k-tile go out one
  // per FOUR MFMAs all the way round: k-tile u+2's pieces 0 .. 11 under k-steps 1 .. 3, 12 .. 15 under k-step 0 of the next trip (the
  // tile prologue issues 16 + 12 pieces to match).  The VMEM port takes 60-180 cycles per piece and two MFMAs are 64: one piece per two
  // MFMAs queued up behind it (K = 4096 forward shapes +4.7 %, profiles/r04_gemm_loop_schedules.txt).  The forms with a k-strided operand
  // (transpose reads: 36 / 48 per k-tile) lose 3 % under it (data gradient 1148 -> 1184, weight gradient frac 0.522 -> 0.537 back
  // on the round-2 order below).
  if constexpr (ROUND) {
  uint32_t offA = OOB, offB = off_of(1, true);
  // one trip = one k-tile.  PEEL_OK: the first trip of a tile is its own copy of the body whose k-step 0 writes the accumulators
  // with a zero C operand -- the 256 v_accvgpr_write per tile and wave that cleared them (in the epilogue: an issue-bound stretch) are
  // gone; the loop behind it runs at least once more (a k-tile past the end reads zeros: K <= 64 pays one empty trip).
  auto trip = [&](auto FIRST_T) {
    const uint32_t bn = bo ^ (uint32_t)(2 * TILE_BYTES);
    tie2<0>(a0, b0);
    mfma_step<decltype(FIRST_T)::value>(acc, a0, b0, [&](int i) {      // (no reads behind the last four MFMAs: they cover the latency of the last reads)
      if (i < 4) { read_frag<1>(a1, i, baseA, bo); read_frag<1>(b1, i, baseB, bo); }
      else if (i < 8) { read_frag<2>(a2, i - 4, baseA, bo); read_frag<2>(b2, i - 4, baseB, bo); }
      else if (i < 12) { read_frag<3>(a3, i - 8, baseA, bo); read_frag<3>(b3, i - 8, baseB, bo); }
      if (i % 4 == 3) dma_c(u + 1, 12 + i / 4, offB);      // the last four pieces of k-tile u+1 (into the other buffer)
      if (i == 12) offA = off_of(u + 2, false);
    });
    tie6<0>(a1, b1, a2, b2, a3, b3);
    __builtin_amdgcn_sched_barrier(0);
    if (!(dbg & 16)) __builtin_amdgcn_s_barrier();
    __builtin_amdgcn_sched_barrier(0);
    mfma_step<false>(acc, a1, b1, [&](int i) {
      if (i % 4 == 1) dma_c(u + 2, i / 4, offA);
    });
    mfma_step<false>(acc, a2, b2, [&](int i) {
      if (i % 4 == 1) dma_c(u + 2, 4 + i / 4, offA);
      if (i == 14) offB = off_of(u + 2, true);
    });
    // k-tile u+1 has landed (its last four pieces went out under k-step 0): only the 8 pieces just issued may be outstanding
    asm volatile("s_waitcnt vmcnt(8)" ::: "memory");
    __builtin_amdgcn_sched_barrier(0);
    if (!(dbg & 16)) __builtin_amdgcn_s_barrier();
    __builtin_amdgcn_sched_barrier(0);
    mfma_step<false>(acc, a3, b3, [&](int i) {      // set 0 of k-tile u+1 in the first half: the second half covers the reads' latency
      if (i < 4) read_frag<0>(a0, i, baseA, bn);
      else if (i < 8) read_frag<0>(b0, i - 4, baseB, bn);
      if (i % 4 == 3) dma_c(u + 2, 8 + i / 4, offB);
    });
    bo = bn;
    ++u;
    };
  if constexpr (PEEL_OK) {
    trip(std::true_type{});
    do { trip(Acc{}); } while (u < n_tiles);
  } else {
    do { trip(Acc{}); } while (u < n_tiles);
  }
  // the reads of "set 0 of the k-tile after the last" are dead, but in flight: their destinations must not be handed out before they land
  tie2<0>(a0, b0);
  return;
  }
  // BLK: the walk, in MFMA gaps that carry nothing else -- the parts NQ (u + 2) .. NQ (u + 2) + NQ - 1 of the walk are k-tile u + 2,
  // whose pieces leave under k-steps 2 and 3 of trip u.  Their indices are taken under k-step 2 of trip u - 1 (the even gaps, between
  // the DMA pieces; in front of the loop for trip 0) and turned into lane offsets under the second half of k-step 1 of trip u.  (In the
  // gaps of k-step 0 of trip u, beside the LDS reads that feed k-step 1, the same work cost 0.6 % of the step: ab_wgrad_ksteps.txt.)  walk_open() and walk_take(q): the two halves of one step of
  // the walk (LiveWalk); walk_offsets(q): part q's two lane offsets.  A part past the count goes out of range through its SCALAR term (OOB_HALF on top of a lane offset inside the
  // window does not wrap): one v_add per offset, no select on a vector.  Part 0 needs no test: where k-tile u + 2 has no part at all
  // nobody reads its buffer (the dense loop's look-ahead reads real rows there too).
  // Both are pure arithmetic, which instruction selection would gather at the top of the trip whatever gap the source names: each
  // starts from and ends in an empty volatile asm on its inputs and results, which keeps it between the gap's neighbours.
  [[maybe_unused]] auto walk_open = [&]() {
    asm volatile("" : "+s"(lw.rest), "+s"(lw.w), "+s"(lw.wi));
    live_open(lw, live_mv);
    asm volatile("" : "+s"(lw.rest), "+s"(lw.w), "+s"(lw.wi));
  };
  [[maybe_unused]] auto walk_take = [&](int q) {
    asm volatile("" : "+s"(lw.w), "+s"(lw.wi), "+s"(lw.cur));
    nextQ[q] = live_take(lw);
    asm volatile("" : "+s"(lw.w), "+s"(lw.cur), "+s"(nextQ[q]));
  };
  [[maybe_unused]] auto walk_offsets = [&](int q) {
    asm volatile("" : "+s"(nextQ[q]));
    const bool has = q == 0 || NQ * (u + 2) + q < n_blk;
    const uint32_t sa = has ? (uint32_t)nextQ[q] * (kstepA >> QSH) : OOB_HALF, sb = has ? (uint32_t)nextQ[q] * (kstepB >> QSH) : OOB_HALF;
    runQA[q] = voffA + sa; runQB[q] = voffB + sb;
    asm volatile("" : "+v"(runQA[q]), "+v"(runQB[q]));
  };
  if constexpr (BLK) {
#pragma unroll
    for (int q = 0; q < NQ; ++q) nextQ[q] = live_next(lw, live_mv);      // k-tile 2's parts; every trip then walks for the one behind it
  }
  do {
    const uint32_t bn = bo ^ (uint32_t)(2 * TILE_BYTES);
    // k-step 0: sets 1 and 2 requested, one fragment behind each MFMA
    tie<0>(a0); tie<0>(b0);
    mfma_step<false, BLK>(acc, a0, b0, [&](int i) {
      if (i < 4) read_frag<1>(a1, i, baseA, bo);
      else if (i < 8) read_frag<1>(b1, i - 4, baseB, bo);
      else if (i < 12) read_frag<2>(a2, i - 8, baseA, bo);
      else read_frag<2>(b2, i - 12, baseB, bo);
    });
    // k-step 1: set 3 requested in the first half; BLK: this trip's offsets in the second
    tie<NR15>(a1); tie<NR15>(b1);
    mfma_step<false, BLK>(acc, a1, b1, [&](int i) {
      if (i < 4) read_frag<3>(a3, i, baseA, bo);
      else if (i < 8) read_frag<3>(b3, i - 4, baseB, bo);
      if constexpr (BLK) { if (i >= 8 && (i - 8) % (8 / NQ) == 0) walk_offsets((i - 8) / (8 / NQ)); }
    });
    // every fragment of k-tile u is in registers: once all waves are here its buffer is free for k-tile u+2
    tie<0>(a2); tie<0>(b2); tie<0>(a3); tie<0>(b3);
    __builtin_amdgcn_sched_barrier(0);
    if (!(dbg & 16)) __builtin_amdgcn_s_barrier();
    __builtin_amdgcn_sched_barrier(0);
    // k-step 2: the A half of k-tile u+2, one piece per two MFMAs (one per three, spread over k-steps 2, 3 and the next trip's
    // k-step 0, measured data gradient +-0, weight gradient -0.9 %: what helps the forward forms does not help these)
    mfma_step<false, BLK>(acc, a2, b2, [&](int i) {
      if (i & 1) dma_run(u + 2, i >> 1);
      if constexpr (BLK) {      // the NEXT trip's walk, one half per gap that carries no DMA piece
        if (i % (8 / NQ) == 0) { const int h = i / (8 / NQ); if (h % 2 == 0) walk_open(); else walk_take(h / 2); }
      }
    });
    // k-step 3: k-tile u+1 has landed (this wave's share: all but the 8 pieces just issued; everybody's: the barrier)
    asm volatile("s_waitcnt vmcnt(8)" ::: "memory");
    __builtin_amdgcn_sched_barrier(0);
    if (!(dbg & 16)) __builtin_amdgcn_s_barrier();
    __builtin_amdgcn_sched_barrier(0);
    mfma_step<false, BLK>(acc, a3, b3, [&](int i) {
      if (i & 1) dma_run(u + 2, 8 + (i >> 1));
      if (!(i & 1)) {
        if (i < 8) read_frag<0>(a0, i >> 1, baseA, bn);
        else read_frag<0>(b0, (i - 8) >> 1, baseB, bn);
      }
    });
    bo = bn;
    ++u;
    // one running lane offset per k-strided operand, opaque to the loop optimiser: left alone it keeps SIXTEEN induction variables
    // (one per piece) and bumps them all in the last MFMA gap of the trip
    if constexpr (!BLK) {      // (BLK: the walk sets its offsets inside the trip)
      if (AKS) { runA += kstepA; asm volatile("" : "+v"(runA)); }
      if (BKS) { runB += kstepB; asm volatile("" : "+v"(runB)); }
    }
  } while (u < n_tiles);
  tie<0>(a0); tie<0>(b0);      // dead, but in flight (see the ROUND loop's exit)
}

// Plain bf16 output (no bias / aux operand): the accumulators are rounded to bf16 BEFORE the trip through LDS, so one pass stages
// 32 rows x 64 columns in 4 KiB (LDS writes run at 64-85 B/clk: they, not the reads or the global stores, are the price of the
// row-major staging) and a lane reads back exactly the 16 bytes it stores.  Same pipelining and accumulator clearing as drain_half.
// WITH_BIAS (k-contiguous B only): bct[ni][q] = the bias of the lane's columns ni*32 + hh*16 + 4q .. +3 (accumulator layout, fetched
// before the main loop), added in fp32 before the rounding.
// ROWS: block mi of the wave's rows starts at row rb.r[mi] (none: its stores leave behind the window), the window covers all of C.
// SLAB: pass it of block mi starts at row rs.r[mi * 4 + it].
template <bool BKS, int NH, bool WITH_BIAS, bool ROWS = false, bool SLAB = false>
IA_DEV void drain_half_plain(const GemmArgs& p, f32x16 (&acc)[4][4], int m0, int n0, char* stg, int lane_e, const f32x4 (&bct)[4][4], float ts = 1.f,
                             RowBlk rb = RowBlk{}, RowSlab rs = RowSlab{}) {
  static_assert(!(WITH_BIAS && BKS), "bias rows are laid out for the k-contiguous B fragment permutation");
  const int hh = lane_e >> 5, li = lane_e & 31, rrow = lane_e >> 3, c8 = lane_e & 7;
  auto stage = [&](int mi) {
    char* const sl = stg + (mi & 1) * 4096;      // two 4-KiB slots per wave: block mi+1 is written while block mi is being read back
#pragma unroll
    for (int ni = 0; ni < 2; ++ni) {
      f32x16& a = acc[mi][NH * 2 + ni];
      if (!BKS) {          // 16 consecutive columns per lane: two 16-byte chunks
#pragma unroll
        for (int h8 = 0; h8 < 2; ++h8) {
          // accumulators live in AGPRs, the conversions are VALU work: copy eight at a time into VGPRs HERE (opaque to the register
          // allocator, which otherwise moves the whole accumulator array into arch VGPRs for the epilogue and spills the main loop): explicit
          // v_accvgpr_read with the source constrained to an AGPR
          f32x4 t0, t1;
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            asm volatile("v_accvgpr_read_b32 %0, %1" : "=v"(t0[j]) : "a"(a[h8 * 8 + j]));
            asm volatile("v_accvgpr_read_b32 %0, %1" : "=v"(t1[j]) : "a"(a[h8 * 8 + 4 + j]));
          }
          // bct arrives multiplied by ts already (ts = the tile's column scale, 1 outside the q columns: a * 1 + b rounds like a + b)
          if (WITH_BIAS) { t0 = t0 * ts + bct[NH * 2 + ni][h8 * 2]; t1 = t1 * ts + bct[NH * 2 + ni][h8 * 2 + 1]; }
          const bf16x8 v = {f2bf(t0[0]), f2bf(t0[1]), f2bf(t0[2]), f2bf(t0[3]), f2bf(t1[0]), f2bf(t1[1]), f2bf(t1[2]), f2bf(t1[3])};
          const int chunk = (ni * 32 + hh * 16 + h8 * 8) >> 3;
          *reinterpret_cast<bf16x8*>(sl + li * 128 + ((chunk ^ (li & 7)) << 4)) = v;
        }
      } else {             // four runs of 4 columns, 8 apart: 8-byte pieces
#pragma unroll
        for (int rg = 0; rg < 4; ++rg) {
          f32x4 t0;
#pragma unroll
          for (int j = 0; j < 4; ++j) asm volatile("v_accvgpr_read_b32 %0, %1" : "=v"(t0[j]) : "a"(a[rg * 4 + j]));
          const bf16x4 v = {f2bf(t0[0]), f2bf(t0[1]), f2bf(t0[2]), f2bf(t0[3])};
          const int col = ni * 32 + rg * 8 + hh * 4;
          *reinterpret_cast<bf16x4*>(sl + li * 128 + (((col >> 3) ^ (li & 7)) << 4) + (col & 7) * 2) = v;
        }
      }
#pragma unroll
      for (int r = 0; r < 16; ++r) a[r] = 0.f;      // dead now: cleared for the next tile in the shadow of the LDS round trip
      __builtin_amdgcn_sched_barrier(0);             // one block at a time: hoisting every accumulator read ran the kernel into scratch
    }
  };
  // Stores through a buffer window over rows m0 .. M-1 of C: a row past M lies behind the window's end and a lane past N starts 2 GiB
  // out, so the hardware drops both -- no execution-mask branches, one 32-bit add per store instead of a 64-bit multiply-add chain
  // (the global_store form of rounds 1-3 spent ~400 scalar / branch / address instructions per wave and tile on clipping that a full
  // tile never needs).  The row advance sits in the LANE offset: the range check does not see a scalar offset.
  const int rows_left = ROWS ? p.M : p.M - m0;
  const uint64_t wbytes = rows_left > 0 ? (uint64_t)rows_left * p.ldc * 2 : 0;
  const __amdgpu_buffer_rsrc_t rsC = ia_rsrc(reinterpret_cast<bf16*>(p.C) + (ROWS ? (size_t)0 : (size_t)m0 * p.ldc), (uint32_t)(wbytes < 0x7FFFFFF0ull ? wbytes : 0x7FFFFFF0ull));
  const int ncol = n0 + c8 * 8;
  const uint32_t voffC = ncol < p.N ? (uint32_t)((rrow * p.ldc + ncol) * 2) : 0x80000000u;
  stage(0);
#pragma unroll
  for (int mi = 0; mi < 4; ++mi) {
    __builtin_amdgcn_wave_barrier();
    const char* const sl = stg + (mi & 1) * 4096;
    u32x4 v[4];
#pragma unroll
    for (int it = 0; it < 4; ++it) {
      const int row = it * 8 + rrow;
      v[it] = *reinterpret_cast<const u32x4*>(sl + row * 128 + ((c8 ^ (row & 7)) << 4));
    }
    __builtin_amdgcn_wave_barrier();
    if (mi < 3) stage(mi + 1);        // the other slot: no wait for the reads above (LDS operations of a wave complete in order)
#pragma unroll
    for (int it = 0; it < 4; ++it) {
      uint32_t off = voffC + (uint32_t)((mi * 32 + it * 8) * p.ldc * 2);
      if constexpr (SLAB) off = rs.r[mi * 4 + it] >= 0 ? voffC + (uint32_t)rs.r[mi * 4 + it] * (uint32_t)(p.ldc * 2) : 0x80000000u;
      else if constexpr (ROWS) off = rb.r[mi] >= 0 ? voffC + (uint32_t)(rb.r[mi] + it * 8) * (uint32_t)(p.ldc * 2) : 0x80000000u;
      if (!IA_GEMM_DBG_HOOKS || !(p.dbg & 64)) __builtin_amdgcn_raw_buffer_store_b128(v[it], rsC, (int)off, 0, 0);
      else asm volatile("" : : "v"(v[it]));
    }
  }
}

// The fused epilogues (bias / residual / GELU / x GELU' / fp32 output) for one 128 x 64 half (NH = 0 / 1) of the wave's 128 x 128 part,
// through the wave's private LDS slots outside the k-tile buffers (no workgroup barrier).  The MFMA C^T fragments give each lane
// 4-element runs scattered over 32 rows, which as direct global stores cost ~11 us per tile (64 separate segments per store
// instruction).  Instead the wave stages 32 rows x 64 columns of fp32 (16-byte chunks XOR-swizzled by row: conflict-free both ways),
// then streams them out: bias / residual / GELU inputs are read and all outputs written as full 128-byte row segments, 8 rows per
// instruction.  C^T fragment: lane (m = li, half hh) register r <-> fragment row i = (r&3) + 8*(r>>2) + 4*hh; k-contiguous B:
// n = hh*16 + r; k-strided B: n = i.
// Slice c (c = 0..15) = rows (c>>2)*32 + ((c>>1)&1)*16 + (c&1)*8 + rrow of the half, the lane's 8 columns n0 + c8*8.  PRE (`full`: the
// half lies entirely inside C, so no row / column guards and the store count of the tile is exact): the bias -- the same 8 columns
// for all slices -- is read once per tile, and the aux operand runs AHEAD slices ahead of the stores: VMEM retires in order, so a load
// issued behind a store can only be waited for by draining that store; issued ahead, hipcc's own counters leave the younger stores in
// flight (vmcnt(2 * AHEAD) in the steady state).
// ROWS: m0 is the wave's first row in the REMAPPED order (it numbers the column-sum partial); block mi lies at row rb.r[mi] of C and aux.
// SLAB: slice c (pass it = c & 3 of block mi = c >> 2) lies at row rs.r[c] of C and aux.
template <int EPI, bool OUTF32, bool BKS, int NH, bool ROWS = false, bool SLAB = false>
IA_DEV void drain_half(const GemmArgs& p, f32x16 (&acc)[4][4], int m0, int n0, char* stg, int lane_e, bool full, bool bias_ready, f32x4 bias_lo,
                       f32x4 bias_hi, RowBlk rb = RowBlk{}, RowSlab rs = RowSlab{}) {
  const int hh = lane_e >> 5, li = lane_e & 31;
  const int rrow = lane_e >> 3, c8 = lane_e & 7;
  constexpr bool HAS_BIAS = EPI == EPI_BIAS || EPI == EPI_BIAS_GELU || EPI == EPI_BIAS_GELU_ACT || EPI == EPI_BIAS_ADD;
  constexpr bool HAS_AUX = EPI == EPI_ADD || EPI == EPI_BIAS_ADD || EPI == EPI_DGELU || EPI == EPI_DGELU_CS;
  constexpr int AHEAD = 4;
  auto drain = [&](auto PREFETCHED) {
    constexpr bool PRE = decltype(PREFETCHED)::value;
    f32x4 pb0, pb1;          // only read when the epilogue has a bias (left undefined otherwise: no registers, no spill)
    float cs[8];
    if (EPI == EPI_DGELU_CS) {      // zeroed here, opaquely: a hoisted zero vector would live (and spill) across the whole main loop
#pragma unroll
      for (int j = 0; j < 8; ++j) asm volatile("v_mov_b32 %0, 0" : "=v"(cs[j]));
    }
    bf16x8 ax[AHEAD + 1];
    // full tiles with bf16 outputs: buffer windows over the wave's rows (from row m0 to the end of the tensor), one lane offset each
    constexpr bool BUF = PRE && !OUTF32;
    const auto window = [&](const void* base, int ld) {
      const uint64_t bytes = (uint64_t)(ROWS ? p.M : p.M - m0) * ld * 2;
      return ia_rsrc(reinterpret_cast<const bf16*>(base) + (ROWS ? (size_t)0 : (size_t)m0 * ld), (uint32_t)(bytes < 0x7FFFFFF0ull ? bytes : 0x7FFFFFF0ull));
    };
    BufIO io{ia_rsrc(nullptr, 0), ia_rsrc(nullptr, 0), 0u};
    __amdgpu_buffer_rsrc_t rsAux = ia_rsrc(nullptr, 0);
    uint32_t voffC = 0, voffAux = 0;
    if (BUF) {
      io.rsC = window(p.C, p.ldc);
      if (EPI == EPI_BIAS_GELU) io.rsC2 = window(p.C2, p.ldc);
      voffC = (uint32_t)((rrow * p.ldc + n0 + c8 * 8) * 2);
      if (HAS_AUX) { rsAux = window(p.aux, p.ldaux); voffAux = (uint32_t)((rrow * p.ldaux + n0 + c8 * 8) * 2); }
    }
    auto aux_of = [&](int c) {
      int row_in = (c >> 2) * 32 + ((c >> 1) & 1) * 16 + (c & 1) * 8;
      if constexpr (SLAB) row_in = rs.r[c];
      else if constexpr (ROWS) row_in = rb.r[c >> 2] + (c & 3) * 8;      // (PRE: every block of a full tile exists)
      if (BUF) return __builtin_bit_cast(bf16x8, __builtin_amdgcn_raw_buffer_load_b128(rsAux, (int)(voffAux + (uint32_t)(row_in * p.ldaux * 2)), 0, 0));
      return *reinterpret_cast<const bf16x8*>(p.aux + (size_t)(m0 + row_in + rrow) * p.ldaux + n0 + c8 * 8);
    };
    if (PRE && HAS_BIAS) {      // normally fetched before the main loop (a load issued here queues behind the previous stores)
      if (bias_ready) { pb0 = bias_lo; pb1 = bias_hi; }
      else { pb0 = *reinterpret_cast<const f32x4*>(p.bias + n0 + c8 * 8); pb1 = *reinterpret_cast<const f32x4*>(p.bias + n0 + c8 * 8 + 4); }
    }
    if (PRE && HAS_AUX) {
#pragma unroll
      for (int c = 0; c < AHEAD; ++c) ax[c] = aux_of(c);
    }
    // One pass = one 32-row block (mi): all 64 lanes stage their 8 quads (32 rows x 64 columns fp32 = 8 KiB, the wave's two 4-KiB
    // slots: with four waves the eight slots of the block are two per wave), then the wave reads them back as rows.  The wave is
    // alone on its SIMD, so the passes are pipelined by hand: the quads of block mi+1 are written as soon as the rows of block mi
    // have been read, and the math / stores of block mi run while that write is in flight.
    auto stage = [&](int mi) {
#pragma unroll
      for (int ni = 0; ni < 2; ++ni)
#pragma unroll
        for (int rg = 0; rg < 4; ++rg) {
          const int chunk = (ni * 32 + (BKS ? rg * 8 + hh * 4 : hh * 16 + rg * 4)) >> 2;
          f32x16& a = acc[mi][NH * 2 + ni];
          const f32x4 v = {a[rg * 4], a[rg * 4 + 1], a[rg * 4 + 2], a[rg * 4 + 3]};
          *reinterpret_cast<f32x4*>(stg + li * 256 + ((chunk ^ (li & 15)) << 4)) = v;
          // the block is dead now: clear it for the next tile here, in the shadow of the LDS round trip (256 accumulator writes in
          // front of the next main loop were ~0.5 us per tile)
          a[rg * 4] = 0.f; a[rg * 4 + 1] = 0.f; a[rg * 4 + 2] = 0.f; a[rg * 4 + 3] = 0.f;
        }
    };
    stage(0);
#pragma unroll
    for (int mi = 0; mi < 4; ++mi) {
      __builtin_amdgcn_wave_barrier();
      f32x4 lo[4], hi[4];
#pragma unroll
      for (int it = 0; it < 4; ++it) {
        const int row = it * 8 + rrow;
        lo[it] = *reinterpret_cast<const f32x4*>(stg + row * 256 + (((2 * c8) ^ (row & 15)) << 4));
        hi[it] = *reinterpret_cast<const f32x4*>(stg + row * 256 + (((2 * c8 + 1) ^ (row & 15)) << 4));
      }
      asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(lo[0]), "+v"(lo[1]), "+v"(lo[2]), "+v"(lo[3]), "+v"(hi[0]), "+v"(hi[1]), "+v"(hi[2]), "+v"(hi[3]));
      __builtin_amdgcn_wave_barrier();
      if (mi < 3) stage(mi + 1);
#pragma unroll
      for (int it = 0; it < 4; ++it) {
        const int row = it * 8 + rrow;
        const int c = mi * 4 + it;
        const int m = SLAB ? rs.r[c] + rrow : (ROWS ? rb.r[mi] + row : m0 + mi * 32 + row), n = n0 + c8 * 8;
        if (PRE) {
          if (HAS_AUX && c + AHEAD < 16) {
            ax[(c + AHEAD) % (AHEAD + 1)] = aux_of(c + AHEAD);
            asm volatile("" ::: "memory");      // the load stays in front of this slice's store (hipcc would sink it behind)
          }
          io.off = voffC + (uint32_t)((SLAB ? rs.r[c] : (ROWS ? rb.r[mi] : mi * 32) + it * 8) * p.ldc * 2);
          if (!(IA_DBG(p) & 64)) epi_store8<EPI, OUTF32, true, BUF, ROWS>(p, m, n, lo[it], hi[it], pb0, pb1, ax[c % (AHEAD + 1)], cs, &io);
        } else {
          if ((!ROWS || (SLAB ? rs.r[c] : rb.r[mi]) >= 0) && m < p.M && n < p.N && !(IA_DBG(p) & 64)) epi_store8<EPI, OUTF32, false, false, ROWS>(p, m, n, lo[it], hi[it], pb0, pb1, ax[0], cs);
        }
        if (IA_DBG(p) & 64) asm volatile("" : : "v"(lo[it]), "v"(hi[it]));
      }
      // GemmArgs::rows_grouped == 2 (block-packed list): block mi closes its group's run when the next slot is empty, belongs to another
      // group, or does not exist -- the same fold as below, the store into THAT group's slot, and the sums start again from zero.  A wave
      // with a block has at least one run, i.e. at least the two stores PEND counts: the counted wait in front of the next tile's
      // main loop only gets stricter by the further ones (wave-uniform conditions: the block rows are scalars).
      if constexpr (ROWS && EPI == EPI_DGELU_CS) {
        if (p.rows_grouped == 2 && rb.r[mi] >= 0 && (mi == 3 || rb.r[mi < 3 ? mi + 1 : 3] < 0 || (rb.r[mi < 3 ? mi + 1 : 3] >> 7) != (rb.r[mi] >> 7))) {
#pragma unroll
          for (int r = 0; r < 8; ++r) {
            float v = cs[r];
            v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(__builtin_bit_cast(int, v), __builtin_bit_cast(int, v), 0x128, 0xF, 0xF, false));
            cs[r] = ia_add_xor32(ia_add_xor16(v));
          }
          if (rrow == 0 && n0 + c8 * 8 < p.N) {
            float* dst = p.csum_part + (size_t)(rb.r[mi] >> 7) * p.N + n0 + c8 * 8;
            gstore16(dst, f32x4{cs[0], cs[1], cs[2], cs[3]});
            gstore16(dst + 4, f32x4{cs[4], cs[5], cs[6], cs[7]});
          }
#pragma unroll
          for (int r = 0; r < 8; ++r) cs[r] = 0.f;
        }
      }
    }
    if (EPI == EPI_DGELU_CS) {
      bool packed = false;
      if constexpr (ROWS) packed = p.rows_grouped == 2;      // (its partials left inside the block loop, fold_store below)
      if (!packed) {
      // column sums of this half's 128 rows: the 8 lanes that share a column group (lane & 7) differ in lane bits 3..5
#pragma unroll
      for (int r = 0; r < 8; ++r) {
        float v = cs[r];
        v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(__builtin_bit_cast(int, v), __builtin_bit_cast(int, v), 0x128, 0xF, 0xF, false));   // row_ror:8 -> lane ^ 8
        v = ia_add_xor32(ia_add_xor16(v));                                                      // lane ^ 16, lane ^ 32 (common.h)
        cs[r] = v;
      }
      int slot = m0 >> 7;
      bool has_slot = true;
      if constexpr (ROWS) {      // group-aligned list: the slot of the group itself (none for a wave whose four blocks do not exist)
        if (p.rows_grouped) { slot = rb.r[0] >> 7; has_slot = rb.r[0] >= 0; }
      }
      if (rrow == 0 && n0 + c8 * 8 < p.N && has_slot) {      // lanes 0..7: 8 consecutive columns each (two 16-byte stores, counted in PEND)
        float* dst = p.csum_part + (size_t)slot * p.N + n0 + c8 * 8;
        gstore16(dst, f32x4{cs[0], cs[1], cs[2], cs[3]});
        gstore16(dst + 4, f32x4{cs[4], cs[5], cs[6], cs[7]});
      }
      }
    }
  };
  if (full && (HAS_BIAS || HAS_AUX) && !(IA_DBG(p) & 256)) drain(std::true_type{}); else drain(std::false_type{});
}

// EPI_ = EPI_NONE_BLK: the plain epilogue behind a k loop over the live 32-row blocks only, two to a trip (GemmArgs::live_blk, an
// ia_kblock_mask; weight-gradient form); EPI_NONE_STP: over the live 16-row steps, four to a trip (live_blk is an ia_kstep_mask).  A value of the epilogue parameter, not a parameter of its own: the other instantiations keep
// their names in profiles and traces.
template <bool AKS, bool BKS, int EPI_, bool OUTF32>
__global__ __launch_bounds__(256) void gemm_kernel(GemmArgs p) {
  constexpr bool STP = EPI_ == EPI_NONE_STP;      // the same walk over 16-row steps, four to a trip
  constexpr bool BLK = EPI_ == EPI_NONE_BLK || STP;
  constexpr bool ROWS = EPI_ >= EPI_ROWS;
  constexpr bool SLAB = EPI_ >= EPI_ROWS + EPI_SLABS;      // the remap in 8-row slabs (EPI_SLABS)
  constexpr int EPI = BLK ? (int)EPI_NONE : (ROWS ? EPI_ - EPI_ROWS - (SLAB ? EPI_SLABS : 0) : EPI_);
  constexpr bool GUARDABLE = ROWS && EPI == EPI_BIAS;      // (tile_blocks)
  static_assert(!SLAB || EPI == EPI_NONE || EPI == EPI_ADD || (!BKS && (EPI == EPI_BIAS || EPI == EPI_BIAS_GELU)), "slab remap: the plain data gradients and three forward forms");
  static_assert(!BLK || (AKS && BKS && OUTF32), "live blocks: the weight-gradient form only");
  static_assert(!ROWS || (!AKS && !OUTF32 && (EPI == EPI_NONE || EPI == EPI_ADD || EPI == EPI_DGELU_CS ||
                                              (!BKS && (EPI == EPI_BIAS || EPI == EPI_BIAS_GELU || EPI == EPI_BIAS_GELU_ACT || EPI == EPI_BIAS_ADD)))),
                "row remap: the data-gradient forms and the k-contiguous forward forms only");
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x, lane0 = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave >> 1, wn = wave & 1;          // 2 x 2 waves, 128 x 128 each, one per SIMD
  const int nk_all = (p.K + BK - 1) / BK;
  // ROWS: the number of M-tiles comes from the device-side list (eight live 32-row blocks per tile); the host sized the grid for every row
  [[maybe_unused]] int n_live = 0;
  if constexpr (ROWS) {
    n_live = __builtin_amdgcn_readfirstlane(p.row_blk[0]);
    p.tiles_m = SLAB ? (n_live + SLAB_TILE - 1) / SLAB_TILE : (n_live + 7) >> 3;
    if constexpr (GUARDABLE && SLAB) {
      if (p.rows_guarded) p.tiles_m = guarded_slab(p, 0, n_live) >= 0 ? 1 : 0;      // (the last live slab lies behind the last whole part, or no tile)
    } else
    if constexpr (GUARDABLE) {
      // one M-tile, or none when no live block lies behind the last whole 128-row part (the usual case: the end of the last sequence
      // is padding) -- every workgroup returns before its first DMA: tile_blocks would have no block to address
      if (p.rows_guarded) {
        const int last = n_live > 0 ? __builtin_amdgcn_readfirstlane(p.row_blk[ROW_BLK_HDR + n_live - 1]) : -1;
        p.tiles_m = last >= ((p.M & ~127) >> 5) ? 1 : 0;
      }
    }
  }
  const int total_tiles = p.tiles_m * p.tiles_n;
  // Split-K launches are a 1-D grid of tiles x splits workgroups whose XCD-aware order has the split OUTERMOST: one XCD's run of
  // 32 work items is then an 8 x 4 block of tiles of ONE k-slab, i.e. 12 operand panel streams per XCD instead of 36 when the
  // splits of a tile shared an XCD (HBM bytes of the fc1 weight gradient: 2.2 GB -> 0.9 GB per launch, algorithmic 0.67 GB).
  int first_tile = blockIdx.x;          // index into the tile work order
  bool ordered = false;                 // first_tile already is a position of that order (no XCD renumbering in coords())
  p.split_id = 0;
  if (p.splits > 1) {
    const int w = xcd_chunk(blockIdx.x, gridDim.x);
    p.split_id = w / total_tiles;
    first_tile = w % total_tiles;
    ordered = true;
  }
  const int kt0 = p.split_id * p.nk_per_split;
  int n_tiles = min(nk_all, kt0 + p.nk_per_split) - kt0;
  // BLK: the 64 mask words of this k-slab, one per lane (the host drops the mask for slabs blk_mask_fits refuses), fetched
  // here -- one vector load pair per lane, waited for on the spot -- so that the k loop's walk over them touches no memory.  A slab starts
  // at any bit of the mask: each lane shifts its 32 bits out of two words, and clips them to the slab's end.
  uint32_t live_mv = 0u;
  [[maybe_unused]] int n_blk = 0;
  if constexpr (BLK) {
    // block bits 2 kt0 .. 2 (kt0 + n_tiles) - 1 of the mask, clipped to the blocks K has; n_tiles becomes the number of PAIRS of live blocks
    // (STP: step bits 4 kt0 .. 4 (kt0 + n_tiles) - 1 of an ia_kstep_mask, clipped to the steps K has; the number of live steps by FOURS)
    constexpr int NQ = STP ? 4 : 2, PSH = STP ? 4 : 5;
    const int nb_all = (p.K + (1 << PSH) - 1) >> PSH, nw = (nb_all + 31) >> 5, first = NQ * kt0 + 32 * lane0, wlo = first >> 5, sh = first & 31;
    const int left = min(NQ * (kt0 + n_tiles), nb_all) - first;
    const uint32_t lo = wlo < nw ? p.live_blk[wlo] : 0u, hi = wlo + 1 < nw ? p.live_blk[wlo + 1] : 0u;
    live_mv = sh ? (lo >> sh) | (hi << (32 - sh)) : lo;
    live_mv = left >= 32 ? live_mv : (left > 0 ? live_mv & ((1u << left) - 1u) : 0u);
    for (uint64_t rest = __ballot(live_mv != 0u); rest; rest &= rest - 1ull)
      n_blk += __builtin_popcount(__builtin_amdgcn_readlane(live_mv, __builtin_ctzll(rest)));
    n_tiles = (n_blk + NQ - 1) / NQ;
  }
  constexpr int PEND = 2 * (16 * epi_stores_per_call<EPI, OUTF32>() + epi_extra_stores<EPI>());   // store instructions of one full-tile epilogue, per wave
  auto coords = [&](int tile, int& bm, int& bn) {
    if (ordered) tile_of_order(p, tile, bm, bn); else tile_of_index(p, tile, total_tiles, bm, bn);
  };
  auto run = [&](int tile, bool prologue_only, f32x16 (&acc)[4][4], bool stores_in_flight) {
    int bm, bn;
    coords(tile, bm, bn);
    int lane = lane0;
    asm volatile("" : "+v"(lane));      // keep per-lane address arithmetic from being hoisted across the tile loop
    RowOff ro{};
    if constexpr (SLAB) ro = slab_offsets<GUARDABLE>(p, bm, wave, n_live);
    else if constexpr (ROWS) {      // a block the list does not have: the tile's first block once more (computed, never stored)
      const Blk8 bl = tile_blocks<GUARDABLE>(p, bm, n_live);
#pragma unroll
      for (int j = 0; j < 8; ++j) ro.o[j] = (uint32_t)(bl.b[j] >= 0 ? bl.b[j] : bl.b[0]) * (uint32_t)(32 * p.lda * 2);
    }
    const uint64_t oa = (uint64_t)(AKS ? kt0 * BK : (ROWS ? 0 : bm * BM)) * p.lda, ob = (uint64_t)(BKS ? kt0 * BK : bn * BN) * p.ldb;
    // (the bf16 bias form keeps 64 bias values in registers across the main loop -- 468 of 512: the peeled first trip spilled there)
    constexpr bool PEEL_OK = !(EPI == EPI_BIAS && !OUTF32 && !BKS);
    main_loop<AKS, BKS, PEND, PEEL_OK, BLK, ROWS, SLAB, STP>(p, smem, acc, rsrc_at(p.A, p.a_bytes, oa), rsrc_at(p.B, p.b_bytes, ob), AKS ? bm * BM : 0, BKS ? bn * BN : 0, kt0,
                              AKS ? 0 : kt0, BKS ? 0 : kt0, n_tiles, nk_all, wm, wn, wave, lane, prologue_only, stores_in_flight, live_mv, ro, n_blk);
  };

  // ---- Dynamic tile claim (persistent launches).  With the static order every workgroup owns the tiles bid, bid + gridDim.x, ...: a
  // workgroup that cannot start -- its CU is held by another stream's kernel (an RCCL all-reduce next to the backward GEMMs: this
  // kernel takes all 160 KiB of LDS, nothing co-resides) -- keeps its 1/256 share hostage until a sibling has finished ALL of its
  // own tiles, i.e. the launch takes two rounds.  Claimed tiles instead: every XCD's contiguous run of the work order (the same runs
  // as before, so the panels still share that XCD's L2) is handed out position by position through one counter per XCD; a workgroup
  // whose own run is exhausted takes from the other XCDs' runs; one that starts late finds nothing left and exits.  Claims run two
  // tiles ahead: issued (wave 0, one lane) in front of a tile's epilogue, read behind the NEXT tile's main loop; an outstanding claim
  // is older than every DMA piece the loops wait for, so their counted vmcnt waits only get stricter by it.
  const bool dyn = p.tile_ctr != nullptr && !ordered;
  const int xcd = blockIdx.x & 7, q8 = total_tiles >> 3, r8 = total_tiles & 7;
  auto run_start = [&](int x) { return x < r8 ? x * (q8 + 1) : r8 * (q8 + 1) + (x - r8) * q8; };
  auto run_len = [&](int x) { return q8 + (x < r8 ? 1 : 0); };
  int* const mailbox = reinterpret_cast<int*>(smem + 2 * 2 * TILE_BYTES);     // wave 0's staging slot, idle outside the epilogue
  uint32_t claimed = 0;
  // (inline asm: handed the builtin, LLVM's atomic optimizer folds the active lanes into one add and consumes the result -- with an
  // s_waitcnt vmcnt(0) -- on the spot, i.e. in front of the main loop, where the previous tile's stores are still draining.  The
  // returned value stays in `claimed` across the main loop; tools/lint_asm_waits.py checks the ISA for any use of that register
  // ahead of the vmcnt(0) in claim_resolve.)
  auto claim_issue = [&]() {
    if (wave == 0 && lane0 == 0)
      // s_nop 4: the counter address may just have been rebuilt by VALU instructions (v_readlane of a spilled SGPR pair) -- a VALU
      // write of an SGPR needs 5 wait states before a VMEM instruction reads it, and the compiler's hazard recogniser does not look
      // inside inline asm (found the hard way: without it the first build's atomic went to a wild address)
      // (the address through readfirstlane: where the compiler keeps the uniform pointer in a VGPR it cannot hand it to an "s" operand)
      {
        const uint64_t a64 = (uint64_t)(p.tile_ctr + xcd);
        const uint32_t alo = __builtin_amdgcn_readfirstlane((uint32_t)a64), ahi = __builtin_amdgcn_readfirstlane((uint32_t)(a64 >> 32));
        const uint64_t addr = ((uint64_t)ahi << 32) | alo;
        asm volatile("s_nop 4\n\tglobal_atomic_add %0, %1, %2, %3 sc0" : "=v"(claimed) : "v"(0u), "v"(1u), "s"(addr) : "memory");
      }
  };
  // -> position in the work order (tile_of_order), or -1: nothing left.  Workgroup-uniform (LDS mailbox between two barriers).
  auto claim_resolve = [&]() -> int {
    // (every wave waits, not only the claimer: behind the main loop nothing but its past-the-end dummy pieces is in flight, and the
    // ISA lint can then see the wait on every path from the atomic)
    asm volatile("s_waitcnt vmcnt(0)" : "+v"(claimed));
    if (wave == 0) {
      int pos = (int)__builtin_amdgcn_readfirstlane(claimed), w = -1;
      if (pos < run_len(xcd)) w = run_start(xcd) + pos;
      else {
        // Own run exhausted (the launch's tail): take from the other XCDs' runs.  One snapshot of the eight counters (lanes 0-7, one
        // load each) tells which runs are used up, so the tail -- where all runs end within a tile time of each other -- costs one load
        // round trip instead of seven returning atomics in a row in front of the last tile's epilogue (+19 % on a 113-us launch).
        uint32_t seen = 0xFFFFFFFFu;
        if (lane0 < 8) seen = __hip_atomic_load(p.tile_ctr + lane0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        const uint32_t mask = (uint32_t)__ballot((int)seen >= q8 + (lane0 < r8 ? 1 : 0)) | (1u << xcd);
        for (int d = 1; d < 8 && w < 0; ++d) {
          const int x = (xcd + d) & 7;
          if ((mask >> x) & 1u) continue;
          uint32_t got = 0;
          if (lane0 == 0) got = __hip_atomic_fetch_add(p.tile_ctr + x, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
          pos = (int)__builtin_amdgcn_readfirstlane(got);
          if (pos < run_len(x)) w = run_start(x) + pos;
        }
      }
      if (lane0 == 0) *reinterpret_cast<volatile int*>(mailbox) = w;
    }
    __syncthreads();
    const int w = __builtin_amdgcn_readfirstlane(*reinterpret_cast<volatile int*>(mailbox));
    __syncthreads();                                                  // wave 0's epilogue writes its staging slot next
    return w;
  };
  auto leave = [&]() {                                                // the last workgroup out re-arms the slot for its next launch
    // every claim of this workgroup has been PERFORMED before it counts itself out (the last one's value may be unused)
    asm volatile("s_waitcnt vmcnt(0)" : "+v"(claimed) : : "memory");
    if (dyn && wave == 0 && lane0 == 0) {
      const uint32_t d = __hip_atomic_fetch_add(p.tile_ctr + 8, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      if (d == gridDim.x - 1) {
#pragma unroll
        for (int i = 0; i < 9; ++i) __hip_atomic_store(p.tile_ctr + i, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      }
    }
  };
  if (dyn) {
    ordered = true;                                                   // `tile` below is a position of the work order
    claim_issue();
    first_tile = claim_resolve();
    if (first_tile < 0) { leave(); return; }
    claim_issue();                                                    // the second tile's claim travels under the first main loop
  }
  if constexpr (ROWS) {
    if (!dyn && first_tile >= total_tiles) return;                    // fewer live tiles than workgroups (none at all: every row is dead)
  }

  f32x16 acc[4][4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;      // later tiles: the epilogue clears every block it has staged
  int tile = first_tile;
  run(tile, true, acc, false);
  bool stores_in_flight = false;
  constexpr bool HAS_BIAS_K = EPI == EPI_BIAS || EPI == EPI_BIAS_GELU || EPI == EPI_BIAS_GELU_ACT || EPI == EPI_BIAS_ADD;
  while (true) {
    int bm, bn;
    coords(tile, bm, bn);
    const int m0_pre = bm * BM + wm * 128, n0_pre = bn * BN + wn * 128;
    const bool full = m0_pre + 128 <= p.M && n0_pre + 128 <= p.N;      // both halves inside C: the store count of the tile is exact
    // the bias of this tile's columns is fetched BEFORE the main loop: VMEM retires in order, so a load issued in the epilogue
    // could only be awaited by draining the stores in front of it (the bias epilogue cost 27 us more than the plain one at
    // 32640 x 4096 x 1024).  Waited for right behind the main loop, where nothing slow is in flight yet.
    // Plain bias + bf16 output: in ACCUMULATOR layout (16 consecutive columns per lane and 32-column block: 64 floats, the wave has
    // 140 spare VGPRs), so the sum is rounded before the LDS trip (drain_half_plain); the other bias epilogues: row layout.
    constexpr bool BIAS_CT = EPI == EPI_BIAS && !OUTF32 && !BKS;
    f32x4 pbv[4] = {};
    f32x4 bct[4][4] = {};
    int lane_b = lane0;
    asm volatile("" : "+v"(lane_b));
    // (ROWS: the bias depends on the columns only, and which rounding an EPI_BIAS element takes -- accumulator layout or row layout --
    // must not depend on where the remap put its row: every wave whose columns lie inside N takes the form a dense full tile takes)
    const bool bias_pre = HAS_BIAS_K && (ROWS ? n0_pre + 128 <= p.N && !(BIAS_CT && p.rows_guarded) : full);
    if (bias_pre && BIAS_CT) {
      const float* bp = p.bias + n0_pre + (lane_b >> 5) * 16;
#pragma unroll
      for (int ni = 0; ni < 4; ++ni)
#pragma unroll
        for (int q = 0; q < 4; ++q) bct[ni][q] = *reinterpret_cast<const f32x4*>(bp + ni * 32 + q * 4);
    } else if (bias_pre) {
      const float* bp = p.bias + n0_pre + (lane_b & 7) * 8;
      pbv[0] = *reinterpret_cast<const f32x4*>(bp); pbv[1] = *reinterpret_cast<const f32x4*>(bp + 4);
      pbv[2] = *reinterpret_cast<const f32x4*>(bp + 64); pbv[3] = *reinterpret_cast<const f32x4*>(bp + 68);
    }
    run(tile, false, acc, stores_in_flight);
    float ts = 1.f;
    if (bias_pre && BIAS_CT) {
#pragma unroll
      for (int ni = 0; ni < 4; ++ni)
        asm volatile("s_waitcnt vmcnt(0)" : "+v"(bct[ni][0]), "+v"(bct[ni][1]), "+v"(bct[ni][2]), "+v"(bct[ni][3]));
      if (n0_pre < p.qcols) {                  // wave-uniform: the 128 columns of this wave lie inside the scaled (q) columns
        ts = p.qscale;
#pragma unroll
        for (int ni = 0; ni < 4; ++ni)
#pragma unroll
          for (int q = 0; q < 4; ++q) bct[ni][q] *= ts;
      }
    } else if (bias_pre) asm volatile("s_waitcnt vmcnt(0)" : "+v"(pbv[0]), "+v"(pbv[1]), "+v"(pbv[2]), "+v"(pbv[3]));
    int next = ordered ? total_tiles : tile + gridDim.x;      // a split-K workgroup owns exactly one (tile, k-slab)
    if (dyn) {
      next = claim_resolve();
      // the claim for the tile AFTER next goes out here, in front of next's prologue DMA and this tile's epilogue: VMEM retires in
      // order, so a claim issued right in front of a main loop holds that loop's first counted wait up for the atomic's round trip
      // (1-3 us under load: +14 % on 25-us tiles at K = 1024, N = 1024); here it has the whole epilogue to come back
      // (issued also when nothing is left -- written as `else claim_issue()` the backend fails with "illegal VGPR to SGPR copy";
      // the stray claim only overshoots a counter, and leave() waits for it before it reports this workgroup done)
      claim_issue();
      if (next < 0) next = total_tiles;
    }
    if (next < total_tiles) run(next, true, acc, false);      // the next tile's first two k-tiles travel under this epilogue

    int lane_e = lane0;
    asm volatile("" : "+v"(lane_e));
    // (the tile origin is known before the main loop now: keep the epilogue's address arithmetic from being scheduled in front of
    // the loop, where it would stay live across it and spill)
    int m0 = m0_pre, n0 = n0_pre;
    asm volatile("" : "+s"(m0), "+s"(n0));
    char* stg = smem + 2 * 2 * TILE_BYTES + wave * 2 * STAGE_BYTES;      // 8 KiB per wave: two staging slots
    bool full_e = full;
    if constexpr (SLAB) {
      // the wave's sixteen slabs, ascending by (block, pass): its part of the tile counts as full (exact store count, unguarded epilogue)
      // when the last of them exists -- then all do -- and is not the partial last slab of M
      const RowSlab rs = slab_rows<GUARDABLE>(p, bm, wm, n_live);
      const bool rows_ok = rs.r[15] >= 0 && rs.r[15] + 8 <= p.M;
      full_e = rows_ok && n0_pre + 128 <= p.N;
      if (!(IA_DBG(p) & 32)) {
        if constexpr (EPI == EPI_NONE) {
          drain_half_plain<BKS, 0, false, true, true>(p, acc, m0, n0, stg, lane_e, bct, 1.f, RowBlk{}, rs);
          drain_half_plain<BKS, 1, false, true, true>(p, acc, m0, n0 + 64, stg, lane_e, bct, 1.f, RowBlk{}, rs);
        } else if (BIAS_CT && bias_pre) {      // (a slab the list does not have, a row past M: the stores fall behind the window)
          if constexpr (BIAS_CT) {
            drain_half_plain<false, 0, true, true, true>(p, acc, m0, n0, stg, lane_e, bct, ts, RowBlk{}, rs);
            drain_half_plain<false, 1, true, true, true>(p, acc, m0, n0 + 64, stg, lane_e, bct, ts, RowBlk{}, rs);
          }
        } else {
          drain_half<EPI, OUTF32, BKS, 0, true, true>(p, acc, m0, n0, stg, lane_e, full_e || (rows_ok && n0 + 64 <= p.N), bias_pre, pbv[0], pbv[1], RowBlk{}, rs);
          drain_half<EPI, OUTF32, BKS, 1, true, true>(p, acc, m0, n0 + 64, stg, lane_e, full_e, bias_pre, pbv[2], pbv[3], RowBlk{}, rs);
        }
      }
    } else
    if constexpr (ROWS) {
      // the wave's four blocks; a tile counts as full (exact store count, unguarded epilogue) when all eight of its blocks exist and
      // none of them is the partial last block of M
      const Blk8 bl = tile_blocks<GUARDABLE>(p, bm, n_live);
      RowBlk rb;
#pragma unroll
      for (int mi = 0; mi < 4; ++mi) rb.r[mi] = (wm ? bl.b[4 + mi] : bl.b[mi]) * 32;      // (-1 -> negative: none)
      bool rows_ok = bl.b[7] >= 0 && bl.b[7] * 32 + 32 <= p.M;
      if constexpr (EPI == EPI_DGELU_CS) {
        // block-packed list: empty slots lie inside a tile.  Their loads and stores fall outside the buffer windows (a negative row: zeros
        // read, nothing written) and still count as issued.  Decided per wave, as the dense kernel decides per 128-row group: the
        // prefetched epilogue when the wave has a block (it then stores at least one partial: the store count PEND stands for) and
        // every group it holds lies inside M whole; the one group M may cut short sits in a wave-row of its own (ia_row_groups_packed)
        // and takes the guarded epilogue, as it does in the dense kernel -- the two paths round the column sums differently (epi_store8)
        if (p.rows_grouped == 2) {
          rows_ok = rb.r[0] >= 0;
#pragma unroll
          for (int mi = 0; mi < 4; ++mi) rows_ok = rows_ok && (rb.r[mi] < 0 || (rb.r[mi] | 127) < p.M);
        }
      }
      full_e = rows_ok && n0_pre + 128 <= p.N;
      if (!(IA_DBG(p) & 32)) {
        if constexpr (EPI == EPI_NONE) {
          drain_half_plain<BKS, 0, false, true>(p, acc, m0, n0, stg, lane_e, bct, 1.f, rb);
          drain_half_plain<BKS, 1, false, true>(p, acc, m0, n0 + 64, stg, lane_e, bct, 1.f, rb);
        } else if (BIAS_CT && bias_pre) {      // (a block the list does not have, a row past M: the stores fall behind the window)
          if constexpr (BIAS_CT) {
            drain_half_plain<false, 0, true, true>(p, acc, m0, n0, stg, lane_e, bct, ts, rb);
            drain_half_plain<false, 1, true, true>(p, acc, m0, n0 + 64, stg, lane_e, bct, ts, rb);
          }
        } else {
          drain_half<EPI, OUTF32, BKS, 0, true>(p, acc, m0, n0, stg, lane_e, full_e || (rows_ok && n0 + 64 <= p.N), bias_pre, pbv[0], pbv[1], rb);
          drain_half<EPI, OUTF32, BKS, 1, true>(p, acc, m0, n0 + 64, stg, lane_e, full_e, bias_pre, pbv[2], pbv[3], rb);
        }
      }
    } else
    if (!(IA_DBG(p) & 32)) {
      if constexpr (EPI == EPI_NONE && !OUTF32) {
        drain_half_plain<BKS, 0, false>(p, acc, m0, n0, stg, lane_e, bct);
        drain_half_plain<BKS, 1, false>(p, acc, m0, n0 + 64, stg, lane_e, bct);
      } else if (BIAS_CT && bias_pre) {
        drain_half_plain<false, 0, BIAS_CT>(p, acc, m0, n0, stg, lane_e, bct, ts);
        drain_half_plain<false, 1, BIAS_CT>(p, acc, m0, n0 + 64, stg, lane_e, bct, ts);
      } else {
        drain_half<EPI, OUTF32, BKS, 0>(p, acc, m0, n0, stg, lane_e, full || (m0 + 128 <= p.M && n0 + 64 <= p.N), bias_pre, pbv[0], pbv[1]);
        drain_half<EPI, OUTF32, BKS, 1>(p, acc, m0, n0 + 64, stg, lane_e, full, bias_pre, pbv[2], pbv[3]);
      }
    }
    if (next >= total_tiles) break;
    // a wave whose 128 x 128 part of the tile was clipped by M or N issued fewer stores than PEND: drain instead of counting
    stores_in_flight = !(IA_DBG(p) & 96) && full_e;
    if (!stores_in_flight) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    tile = next;
  }
  leave();
}

}  // namespace t256w



// ============================================================================== T256LA (round 6): T256W with a k pipeline that never drains
// Plain NT form only (k-contiguous A and B, bf16 output, no bias / aux operand), static tile order, one workgroup per CU.  T256W ends
// every tile with an empty pipeline: the last two trips of its k loop fetch past the end, the next tile starts with a burst of 28 DMA
// pieces (~41 cycles of blocked issue each), a wait, a workgroup barrier and the exposed latency of its first fragment reads.  Here the
// last two trips fetch the NEXT tile's k-tiles 0 and 1 (a second descriptor pair, chosen by scalar selects), so when a tile's last trip
// ends the next tile's k-tile 0 sits in LDS, its first fragment set is already requested (what T256W reads as "dead" look-ahead), and
// k-tile 1 is in flight: the drain runs, and the next tile's first trip starts where a steady-state trip would -- no prologue burst, no
// prologue wait, no barrier, no exposed read.  The loop-carried pipeline state is the fragment set a0 / b0 (32 VGPRs, live across the
// drain: the plain kernel has ~100 to spare there) and the LDS buffer parity.  One tile boundary = drain only.
namespace t256la {
using namespace t256w;

// ROWS (GemmArgs::row_blk, see EPI_ROWS): an M-tile is eight entries of the live-block list.  A's windows cover the whole operand (empty
// behind the last tile, as before) and every A piece takes its row offset -- the current tile's or the next one's -- as a scalar.
// SLAB (EPI_SLABS): an M-tile is 32 entries of a slab list, and the row offsets are this wave's own.
template <bool ROWS>
__global__ __launch_bounds__(256) void gemm_kernel(GemmArgs p) {
  constexpr bool SLAB = false;
#include "gemm_t256la_body.inc"
}
__global__ __launch_bounds__(256) void gemm_slab_kernel(GemmArgs p) {
  constexpr bool ROWS = true, SLAB = true;
#include "gemm_t256la_body.inc"
}
}  // namespace t256la

// Optional per-launch timing of ONE kernel instantiation with HIP events on the launch stream
// (bench.py's roofline leg): variant id = AKS*1000 + BKS*100 + EPI*10 + OUTF32.
struct GemmProf {
  bool on = false;
  int variant = -1, n = 0, cap = 0;
  double flops = 0.0, bytes = 0.0;      // algorithmic: 2 M N K, and A + B read once + C written once
  hipEvent_t* ev = nullptr;
};
GemmProf g_prof;

// C[m][n] (+)= sum_s ws[s][m][n]
// out[group * M + m] += sum_s rsum_ws[group][s][m]: workgroup x of a group folds m = 32x .. 32x+31 (workgroups beyond M/32 skip it);
// 8 lanes per m, lane l adds partials l, l+8, ... in order and lane 0 folds the 8 lane sums in order (fixed order -> deterministic)
IA_DEV void fold_row_sums(const float* rsum_ws, float* rsum_out, int M, int splits) {
  __shared__ float rs[256];
  if (!rsum_ws || (int)blockIdx.x * 32 >= M) return;          // uniform per workgroup
  const int lane = threadIdx.x & 7, m = blockIdx.x * 32 + (threadIdx.x >> 3);
  float a = 0.f;
  if (m < M)
    for (int sp = lane; sp < splits; sp += 8) a += rsum_ws[((size_t)blockIdx.y * splits + sp) * M + m];
  rs[threadIdx.x] = a;
  __syncthreads();
  if (lane == 0 && m < M) {
    float sum = rs[threadIdx.x];
#pragma unroll
    for (int l = 1; l < 8; ++l) sum += rs[threadIdx.x + l];
    rsum_out[(size_t)blockIdx.y * M + m] += sum;
  }
  __syncthreads();
}

__global__ __launch_bounds__(256) void splitk_reduce_kernel(const float* __restrict__ ws, float* __restrict__ C, int M, int N, int ldc,
                                                            int splits, int accumulate, long gc, const float* rsum_ws, float* rsum_out) {
  fold_row_sums(rsum_ws, rsum_out, M, splits);
  ws += (size_t)blockIdx.y * splits * M * N;       // blockIdx.y = channel group of a batched convolution GEMM
  C += (size_t)blockIdx.y * gc;
  const size_t total4 = (size_t)M * N / 4;
  for (size_t t = (size_t)blockIdx.x * 256 + threadIdx.x; t < total4; t += (size_t)gridDim.x * 256) {
    const size_t e = t * 4;
    const int m = (int)(e / N), n = (int)(e % N);
    f32x4 acc = *reinterpret_cast<const f32x4*>(ws + e);
    for (int s = 1; s < splits; ++s) acc += *reinterpret_cast<const f32x4*>(ws + (size_t)s * M * N + e);
    float* c = C + (size_t)m * ldc + n;
    if (accumulate) acc += *reinterpret_cast<const f32x4*>(c);
    *reinterpret_cast<f32x4*>(c) = acc;
  }
}

// the same sum for deep cuts (conv weight gradients: hundreds of partials of a few KB each): 8 lanes share one output quad,
// lane l adds partials l, l+8, ... in order and lane 0 folds the 8 lane sums in order (fixed order -> deterministic)
__global__ __launch_bounds__(256) void splitk_reduce_deep_kernel(const float* __restrict__ ws, float* __restrict__ C, int M, int N, int ldc,
                                                                 int splits, int accumulate, long gc, const float* rsum_ws, float* rsum_out) {
  __shared__ f32x4 red[256];
  fold_row_sums(rsum_ws, rsum_out, M, splits);
  ws += (size_t)blockIdx.y * splits * M * N;
  C += (size_t)blockIdx.y * gc;
  const size_t total4 = (size_t)M * N / 4;
  const int lane = threadIdx.x & 7;
  const size_t t = (size_t)blockIdx.x * 32 + (threadIdx.x >> 3);
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
  if (t < total4)
    for (int sp = lane; sp < splits; sp += 8) acc += *reinterpret_cast<const f32x4*>(ws + (size_t)sp * M * N + t * 4);
  red[threadIdx.x] = acc;
  __syncthreads();
  if (lane == 0 && t < total4) {
    f32x4 sum = red[threadIdx.x];
#pragma unroll
    for (int l = 1; l < 8; ++l) sum += red[threadIdx.x + l];
    const size_t e = t * 4;
    float* c = C + (size_t)(e / N) * ldc + (e % N);
    if (accumulate) sum += *reinterpret_cast<const f32x4*>(c);
    *reinterpret_cast<f32x4*>(c) = sum;
  }
}

struct Plan { bool big; int splits; };

// Tile choice + split-K factor.  Weight-gradient GEMMs have outputs of only a few dozen tiles (1024x1024 ->
// 16 tiles of 256x256) while K = #tokens is tens of thousands, so K is cut until every CU has a workgroup.
Plan make_plan(int M, int N, int K, bool f32_out, int groups = 1) {
  Plan pl;
  const int nk = (K + BK - 1) / BK;
  const long t256n = (long)((M + 255) / 256) * ((N + 255) / 256);
  const int smax = f32_out ? (nk / 8 > 32 ? 32 : (nk / 8 < 1 ? 1 : nk / 8)) : 1;
  pl.big = M >= 256 && N >= 256 && (N & 7) == 0 && t256n * smax >= 160;
  if (groups > 1) pl.big = false;
  const long tiles = pl.big ? t256n : (long)((M + 127) / 128) * ((N + 127) / 128) * groups;
  // Pick the cut that minimises the makespan: ceil(workgroups / resident slots) rounds of (k-tiles per workgroup + a fixed
  // prologue/epilogue cost), plus the fixed-order reduction that reads one fp32 copy of C per split.  Overshooting the
  // slot count by a few workgroups (36 tiles x 8 = 288 on 256 CUs) would cost a whole extra round.
  const long slots = pl.big ? 256 : 512;
  // outputs of one or two tiles under a huge K (convolution weight gradients: 64 x 576 over millions of pixels) are pure
  // streaming reads: cut K until the resident slots are full, the partials are a few KB each
  int smax2 = smax;
  if (f32_out && slots / tiles > smax2) { smax2 = (int)(slots / tiles); if (smax2 > nk / 8) smax2 = nk / 8 < 1 ? 1 : nk / 8; if (smax2 < smax) smax2 = smax; }
  const double reduce_per_split = (double)tiles * (pl.big ? 0.0244 : 0.0061);   // in k-tile times of one workgroup
  int best = 1;
  double best_cost = 1e30;
  for (int s = 1; s <= smax2; ++s) {
    const long rounds = (tiles * s + slots - 1) / slots;
    const double cost = (double)rounds * ((nk + s - 1) / s + 6) + (s > 1 ? s * reduce_per_split : 0.0);
    if (cost < best_cost - 1e-9) { best_cost = cost; best = s; }
  }
  pl.splits = best;
  return pl;
}

// Counter slot of the next dynamic-claim launch (nullptr: static order).  File-scope state: `launch` is a template, its function-local
// statics would exist once per instantiation -- and two instantiations running on two streams would share slot 0.
// Host threads may launch concurrently (ctypes releases the GIL): the sequence is atomic, so two launches never share a slot, and the
// counter array's address is kept per device (a __device__ symbol has one instance per device).  A slot comes round again after
// CTR_SLOTS launches of this process; the kernel's last workgroup re-arms it, so a reuse is only unsafe while >= CTR_SLOTS persistent
// GEMM launches are in flight at once -- the step has ~400 of them in total, each queue holds far fewer.
int g_dynamic = -1;
constexpr int MAX_DEVICES = 16;
uint32_t* g_ctr_base[MAX_DEVICES] = {};
std::atomic<unsigned> g_launch_seq{0};
uint32_t* next_ctr_slot() {
  // Default: the static order.  The claims cost the 256-wide GEMMs 0-1.5 % (two workgroup barriers per tile; 14 % on a 113-us launch of
  // four 25-us tiles per workgroup) and buy nothing while no other stream holds CUs; the data-parallel host switches them on when it
  // creates a communicator (dist.init_from_env at world size > 1 -> ia_debug_gemm_dynamic(1)), IA_GEMM_DYNAMIC=0/1 forces either.
  if (g_dynamic < 0) {
    const char* e = getenv("IA_GEMM_DYNAMIC");
    g_dynamic = e ? atoi(e) : 0;
  }
  if (!g_dynamic) return nullptr;
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= MAX_DEVICES) return nullptr;
  uint32_t* base = __atomic_load_n(&g_ctr_base[dev], __ATOMIC_ACQUIRE);
  if (!base) {
    if (hipGetSymbolAddress((void**)&base, HIP_SYMBOL(g_tile_ctr)) != hipSuccess || !base) return nullptr;
    __atomic_store_n(&g_ctr_base[dev], base, __ATOMIC_RELEASE);
  }
  return base + (size_t)(g_launch_seq.fetch_add(1u, std::memory_order_relaxed) % CTR_SLOTS) * CTR_WORDS;
}

// EPI_ROWS launches: the rows of the dead 32-row blocks of C (bf16 [M, N], N a multiple of 8) written as zeros -- not every consumer of a
// data gradient filters its rows -- and, with column-sum partials, the partial rows behind the last remapped M-tile (the second stage
// sums a row count the host knows: one pair per 256 rows of M).  Dead blocks and partial rows are dealt out over the grid.
// grouped (a group-aligned list, GemmArgs::rows_grouped): the partial rows zeroed are the slots of the dead 128-row groups (the first block of
// each names it) and the slots behind the last group of M.
__global__ __launch_bounds__(256) void zero_dead_rows_kernel(const int* __restrict__ list, bf16* __restrict__ C, int ldc, int M, int N,
                                                             float* __restrict__ csum_part, int part_rows, int grouped = 0) {
  const int n_live = list[0], n_dead = list[1], nbr = (list[2] + 7) & ~7;
  const int* dead = list + t256w::ROW_BLK_HDR + nbr;
  const int n8 = N >> 3;
  const u32x4 z = {0u, 0u, 0u, 0u};
  for (int d = blockIdx.x; d < n_dead; d += gridDim.x) {
    const int r0 = dead[d] * 32;
    for (int i = threadIdx.x; i < 32 * n8; i += 256) {
      const int r = r0 + i / n8, c = (i % n8) * 8;
      if (r < M) *reinterpret_cast<u32x4*>(C + (size_t)r * ldc + c) = z;
    }
  }
  if (csum_part && grouped == 2) {      // block-packed list: every slot (a group without a live block stores none)
    const size_t total = (size_t)part_rows * N;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) csum_part[i] = 0.f;
  } else if (csum_part && grouped) {
    const int ngrp = (M + 127) >> 7;
    for (int d = blockIdx.x; d < n_dead + (part_rows - ngrp); d += gridDim.x) {
      const int g = d < n_dead ? ((dead[d] & 3) ? -1 : dead[d] >> 2) : ngrp + (d - n_dead);
      if (g < 0) continue;
      for (int i = threadIdx.x; i < N; i += 256) csum_part[(size_t)g * N + i] = 0.f;
    }
  } else if (csum_part) {
    const int first = ((n_live + 7) >> 3) * 2;
    const size_t total = part_rows > first ? (size_t)(part_rows - first) * N : 0;
    float* base = csum_part + (size_t)first * N;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) base[i] = 0.f;
  }
}

// EPI_SLABS launches: the same for a slab list (ia_row_slabs) -- the rows of its dead 8-row slabs written as zeros, dealt out over the grid
// (a workgroup takes four slabs at a time: the 32 rows the block form's fill takes).
__global__ __launch_bounds__(256) void zero_dead_slabs_kernel(const int* __restrict__ list, bf16* __restrict__ C, int ldc, int M, int N) {
  const int n_dead = list[1], nsr = (list[2] + t256w::SLAB_TILE - 1) & ~(t256w::SLAB_TILE - 1);
  const int* dead = list + t256w::ROW_BLK_HDR + nsr;
  const int n8 = N >> 3;
  const u32x4 z = {0u, 0u, 0u, 0u};
  for (int d0 = blockIdx.x * 4; d0 < n_dead; d0 += gridDim.x * 4) {
    const int nd = n_dead - d0 < 4 ? n_dead - d0 : 4;
    for (int i = threadIdx.x; i < nd * 8 * n8; i += 256) {
      const int rr = i / n8, r = dead[d0 + (rr >> 3)] * 8 + (rr & 7), c = (i % n8) * 8;
      if (r < M) *reinterpret_cast<u32x4*>(C + (size_t)r * ldc + c) = z;
    }
  }
}

// the 256-wide kernels one instantiation of `launch` may start: each needs its dynamic LDS size set once
enum KernelForm {
  FORM_T256W,            // this instantiation of t256w
  FORM_T256LA,           // the look-ahead kernel
  FORM_ROWS_T256W,       // the row remap (32-row blocks) of FORM_T256W ...
  FORM_ROWS_T256LA,      // ... and of FORM_T256LA
  FORM_WGRAD_KBLOCKS,    // the live-block weight gradient
  FORM_WGRAD_KSTEPS,     // the live-step weight gradient
  FORM_SLABS_T256W,      // the slab remap of FORM_T256W ...
  FORM_SLABS_T256LA,     // ... and of FORM_T256LA
  FORM_COUNT
};

// kind: what a.row_blk points at (SLABS: a slab list, ia_row_slabs; else a list of 32-row blocks), and what a.live_blk does (KSTEPS: an
// ia_kstep_mask; else an ia_kblock_mask)
template <bool AKS, bool BKS, int EPI, bool OUTF32>
int launch(GemmArgs a, bool big, hipStream_t st, IaRowFilter::Kind kind = IaRowFilter::NONE) {
  constexpr int vid = AKS * 1000 + BKS * 100 + EPI * 10 + (OUTF32 ? 1 : 0);
  // the forms that may carry a block list (GemmArgs::row_blk): the data gradients, and the forward epilogues on k-contiguous operands
  constexpr bool DROWS = !AKS && !OUTF32 && (EPI == EPI_NONE || EPI == EPI_ADD || EPI == EPI_DGELU_CS ||
                                             (!BKS && (EPI == EPI_BIAS || EPI == EPI_BIAS_GELU || EPI == EPI_BIAS_GELU_ACT || EPI == EPI_BIAS_ADD)));
  // (a launch over the live blocks only is not recorded: the host cannot know how many blocks it executed, and the recorded FLOPs are
  // those of launches that executed all of theirs)
  constexpr bool WGRAD = AKS && BKS && EPI == EPI_NONE && OUTF32;      // the form that may carry a live-block mask (GemmArgs::live_blk)
  const bool rec = g_prof.on && g_prof.variant == vid && g_prof.n < g_prof.cap && !(WGRAD && a.live_blk) && !(DROWS && a.row_blk);
  if (rec) (void)hipEventRecord(g_prof.ev[2 * g_prof.n], st);
  if (big) {
    a.tiles_m = (a.M + t256w::BM - 1) / t256w::BM; a.tiles_n = (a.N + t256w::BN - 1) / t256w::BN;
    if (a.row_blk && a.rows_guarded) a.tiles_m = 1;      // (the launch over the last blocks of the list: one M-tile, one workgroup per N-tile)
    const int ntile = a.tiles_m * a.tiles_n;
    // split-K: one workgroup per (tile, k-slab), 1-D so the kernel can order them XCD-aware with the slab outermost;
    // otherwise persistent over tiles, one workgroup per CU
    const int gx = a.splits > 1 ? ntile * a.splits : (ntile < 256 ? ntile : 256);
    // persistent launches with more than one tile per workgroup claim their tiles dynamically (IA_GEMM_DYNAMIC=0: the static order)
    a.tile_ctr = (a.splits == 1 && ntile > gx) ? next_ctr_slot() : nullptr;
    void (*kern)(GemmArgs) = t256w::gemm_kernel<AKS, BKS, EPI, OUTF32>;
    static bool attr_set[FORM_COUNT] = {};
    KernelForm form = FORM_T256W;
    if constexpr (WGRAD) {
      if (a.live_blk && kind == IaRowFilter::KSTEPS) { kern = t256w::gemm_kernel<true, true, EPI_NONE_STP, true>; form = FORM_WGRAD_KSTEPS; }
      else if (a.live_blk) { kern = t256w::gemm_kernel<true, true, EPI_NONE_BLK, true>; form = FORM_WGRAD_KBLOCKS; }
    }
    // plain NT form, several tiles per workgroup, static order: the look-ahead kernel (t256la; IA_GEMM_LA=0 keeps t256w)
    if constexpr (!AKS && !BKS && EPI == EPI_NONE && !OUTF32) {
      const char* e = getenv("IA_GEMM_LA");       // (read per launch: tests and A/B runs switch it in one process)
      if ((e ? atoi(e) : 1) && a.splits == 1 && ntile > gx && !a.tile_ctr && a.K >= 2 * BK && !(IA_DBG(a))) { kern = t256la::gemm_kernel<false>; form = FORM_T256LA; }
    }
    // over the live 32-row blocks: the remapped form of the kernel chosen above, dead rows zeroed first where the caller asks for it
    if constexpr (DROWS) {
      constexpr bool DSLABS = EPI == EPI_NONE || EPI == EPI_ADD || (!BKS && (EPI == EPI_BIAS || EPI == EPI_BIAS_GELU));
      const bool la = form == FORM_T256LA;
      if (a.row_blk && kind == IaRowFilter::SLABS) {
        if constexpr (DSLABS) {
          if (la) kern = t256la::gemm_slab_kernel;
          else kern = t256w::gemm_kernel<false, BKS, EPI_ROWS + EPI_SLABS + EPI, false>;
          form = la ? FORM_SLABS_T256LA : FORM_SLABS_T256W;
          if (a.rows_fill) hipLaunchKernelGGL(zero_dead_slabs_kernel, dim3(1024), dim3(256), 0, st, a.row_blk, (bf16*)a.C, a.ldc, a.fill_m, a.N);
          if (a.rows_fill && EPI == EPI_BIAS_GELU) hipLaunchKernelGGL(zero_dead_slabs_kernel, dim3(1024), dim3(256), 0, st, a.row_blk, a.C2, a.ldc, a.fill_m, a.N);
        } else return IA_ERR_UNSUPPORTED;
      } else if (a.row_blk) {
        if (la) kern = t256la::gemm_kernel<true>;      // (the look-ahead kernel's remapped form where the dense call takes that kernel)
        else kern = t256w::gemm_kernel<false, BKS, EPI_ROWS + EPI, false>;
        form = la ? FORM_ROWS_T256LA : FORM_ROWS_T256W;
        if (a.rows_fill)
          hipLaunchKernelGGL(zero_dead_rows_kernel, dim3(1024), dim3(256), 0, st, a.row_blk, (bf16*)a.C, a.ldc, a.fill_m, a.N, a.csum_part, ((a.M + 255) / 256) * 2,
                             a.rows_grouped);
        if (a.rows_fill && EPI == EPI_BIAS_GELU)
          hipLaunchKernelGGL(zero_dead_rows_kernel, dim3(1024), dim3(256), 0, st, a.row_blk, a.C2, a.ldc, a.fill_m, a.N, (float*)nullptr, 0);
      }
    }
    if (!attr_set[form]) {
      if (hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, t256w::LDS_BYTES) != hipSuccess) return IA_ERR_LAUNCH;
      attr_set[form] = true;
    }
    hipLaunchKernelGGL(kern, dim3(gx), dim3(256), t256w::LDS_BYTES, st, a);
  } else {
    a.tiles_m = (a.M + t128::BM - 1) / t128::BM; a.tiles_n = (a.N + t128::BN - 1) / t128::BN;
    hipLaunchKernelGGL((t128::gemm_kernel<AKS, BKS, EPI, OUTF32>), dim3(a.tiles_m * a.tiles_n * a.splits * a.groups), dim3(256), 0, st, a);
  }
  if (OUTF32 && a.splits > 16) {
    size_t g = ((size_t)a.M * a.N / 4 + 31) / 32;
    if (a.rsum_out && g < (size_t)(a.M + 31) / 32) g = (size_t)(a.M + 31) / 32;
    hipLaunchKernelGGL(splitk_reduce_deep_kernel, dim3((unsigned)g, a.groups), dim3(256), 0, st, a.ws, (float*)a.C, a.M, a.N, a.ldc, a.splits,
                       a.accumulate, a.gc, a.rsum_out ? a.rsum_ws : nullptr, a.rsum_out);
  } else if (OUTF32 && a.splits > 1) {
    size_t g = ((size_t)a.M * a.N / 4 + 255) / 256; if (g > 4096) g = 4096;
    if (a.rsum_out && g < (size_t)(a.M + 31) / 32) g = (size_t)(a.M + 31) / 32;      // fold_row_sums: one workgroup per 32 rows
    hipLaunchKernelGGL(splitk_reduce_kernel, dim3((int)g, a.groups), dim3(256), 0, st, a.ws, (float*)a.C, a.M, a.N, a.ldc, a.splits, a.accumulate,
                       a.gc, a.rsum_out ? a.rsum_ws : nullptr, a.rsum_out);
  }
  if (rec) {
    (void)hipEventRecord(g_prof.ev[2 * g_prof.n + 1], st);
    g_prof.flops += 2.0 * a.M * a.N * a.K;
    g_prof.bytes += 2.0 * ((double)a.M * a.K + (double)a.N * a.K) + (OUTF32 ? 4.0 : 2.0) * a.M * a.N;
    ++g_prof.n;
  }
  return ia_check_launch();
}

}  // namespace

// workspace an fp32-output GEMM can use for split-K partial sums (0 = none needed)
extern "C" size_t ia_gemm_workspace_bytes(int M, int N, int K, int c_is_f32) {
  if (!c_is_f32 || M <= 0 || N <= 0 || K <= 0) return 0;
  const Plan pl = make_plan(M, N, K, true);
  return pl.splits > 1 ? (size_t)pl.splits * M * (N + 1) * sizeof(float) : 0;      // + the row-sum partials of the weight-gradient form
}

// One GEMM call as the host entry points describe it (host only: GemmArgs is what the kernels see).  The operands, output and shape as in
// ia_gemm_bf16; everything else is optional.
struct GemmCall {
  const void* A; int a_kstrided, lda;
  const void* B; int b_kstrided, ldb;
  void* C; int c_is_f32, ldc;
  int M, N, K;
  int epilogue = EPI_NONE;
  const float* bias = nullptr;
  const void* aux = nullptr; int ldaux = 0;
  void* C2 = nullptr;
  int accumulate = 0;
  void* workspace = nullptr; size_t workspace_bytes = 0;
  const IaViewGemm* view = nullptr;      // ia_gemm_view: shifted operand views, channel groups
  int qcols = 0; float qscale = 1.f;     // ia_gemm_bf16_qscale: the first qcols columns leave multiplied by qscale
  IaRowFilter filter;                    // the live rows (a list) or the live k (a mask); honoured by the forms that have a filtered kernel
  bool tail = false;                     // gemm_core's own second launch for the scaled-column tail (see there)
};
static int gemm_core(const GemmCall& c, hipStream_t stream);

// workspace of an IA_EPI_DGELU_COLSUM GEMM: one fp32 row of N partial sums per 128-row block of the output (and never less than
// the stand-alone column-sum kernel needs, which small shapes fall back to)
extern "C" size_t ia_gemm_colsum_workspace_bytes(int M, int N) {
  if (M <= 0 || N <= 0) return 0;
  const size_t fused = (size_t)((M + 255) / 256) * 2 * N * sizeof(float), plain = ia_colsum_workspace_bytes(M, N);
  return fused > plain ? fused : plain;
}

extern "C" int ia_gemm_bf16(const void* A, int a_kstrided, int lda, const void* B, int b_kstrided, int ldb,
                            void* C, int c_is_f32, int ldc, int M, int N, int K, int epilogue,
                            const float* bias, const void* aux, int ldaux, void* C2, int accumulate, void* workspace,
                            size_t workspace_bytes, hipStream_t stream) {
  GemmCall c{A, a_kstrided, lda, B, b_kstrided, ldb, C, c_is_f32, ldc, M, N, K};
  c.epilogue = epilogue; c.bias = bias; c.aux = aux; c.ldaux = ldaux; c.C2 = C2; c.accumulate = accumulate;
  c.workspace = workspace; c.workspace_bytes = workspace_bytes;
  return gemm_core(c, stream);
}

// IA_EPI_BIAS GEMM (k-contiguous operands, bf16 output) whose first scaled_cols columns (a multiple of 128) are multiplied by col_scale
// after the bias: the fused QKV projection of the encoder layers, q leaving as q * softmax scale * log2 e (GemmArgs::qcols)
extern "C" int ia_gemm_bf16_qscale(const void* A, int lda, const void* B, int ldb, void* C, int ldc, int M, int N, int K, const float* bias,
                                   int scaled_cols, float col_scale, hipStream_t stream) {
  return ia_gemm_fwd_filtered(A, lda, B, ldb, C, ldc, M, N, K, EPI_BIAS, bias, nullptr, 0, nullptr, scaled_cols, col_scale, IaRowFilter{}, stream);
}

// ---- data gradient over the live 32-row blocks only
// The remapped kernel addresses A, C and aux through one 32-bit buffer window each that covers the whole tensor, 16 bytes per lane.
static bool dgrad_rows_fit(int M, int lda, int ldc, int ldaux) {
  const uint64_t lim = 0x7FFFFFF0ull, rows = (uint64_t)M + 32;
  return rows * lda * 2 < lim && rows * ldc * 2 < lim && rows * (uint64_t)ldaux * 2 < lim && !(ldc & 7) && !(ldaux & 7);
}
// block t = rows 32t .. 32t+31 (clipped to M): live = any row_live set.  One function for the device kernel and the host entry.
// gshift = 2 (ia_row_groups): live = any row_live set in the block's 128-row GROUP (rows 128 (t >> 2) .. + 127, clipped to M), so the live
// blocks come as the four blocks of each live group.
static __host__ __device__ inline bool row_block_live(const uint8_t* row_live, int M, int t, int gshift = 0) {
  const int len = 32 << gshift, r0 = (t >> gshift) * len;
  const uint8_t* r = row_live + (size_t)r0;
  const int n = M - r0 < len ? M - r0 : len;
  uint64_t any = 0;
  if (n == len && ((uintptr_t)r & 7) == 0) {
    for (int i = 0; i < len / 8; ++i) any |= reinterpret_cast<const uint64_t*>(r)[i];
  } else {
    for (int i = 0; i < n; ++i) any |= r[i];
  }
  return any != 0;
}
namespace {
inline size_t al256(size_t b) { return (b + 255) & ~(size_t)255; }
// One wave, no LDS (a workgroup that asks for none can start beside the persistent GEMM workgroups of another stream, which hold all of
// a CU's LDS).  Lane l looks at blocks 64i + l: first the flags of up to 64 rounds i are gathered into one 64-bit word per lane (loads
// only, so they overlap), then every round is one ballot: a block's place in the live list is the number of live blocks in front of it,
// in the dead list the number of dead ones (t minus that).
__global__ __launch_bounds__(64) void row_blocks_kernel(const uint8_t* __restrict__ row_live, int M, int nb, int* __restrict__ out, int gshift) {
  const int nbr = (nb + 7) & ~7;
  int* const live = out + t256w::ROW_BLK_HDR;
  int* const dead = live + nbr;
  const int lane = threadIdx.x;
  int base = 0;
  for (int c0 = 0; c0 < nb; c0 += 64 * 64) {
    uint64_t flags = 0;
#pragma unroll 8
    for (int i = 0; i < 64; ++i) {
      const int t = c0 + i * 64 + lane;
      if (t < nb && row_block_live(row_live, M, t, gshift)) flags |= 1ull << i;
    }
    for (int i = 0; i < 64 && c0 + i * 64 < nb; ++i) {
      const int t = c0 + i * 64 + lane;
      const bool lv = (flags >> i) & 1ull;
      const uint64_t b = __ballot(lv);
      const int at = base + __popcll(b & ((1ull << lane) - 1ull));
      if (t < nb) { if (lv) live[at] = t; else dead[t - at] = t; }
      base += __popcll(b);
    }
  }
  if (lane < t256w::ROW_BLK_HDR) out[lane] = lane == 0 ? base : (lane == 1 ? nb - base : (lane == 2 ? nb : 0));
}
}  // namespace

extern "C" size_t ia_row_blocks_bytes(int M_rows) {
  if (M_rows <= 0) return 0;
  const size_t nbr = (size_t)(((M_rows + 31) / 32 + 7) & ~7);
  return (t256w::ROW_BLK_HDR + 2 * nbr) * sizeof(int);
}
extern "C" int ia_row_blocks(const uint8_t* row_live, int M_rows, int* list, hipStream_t stream) {
  (void)hipGetLastError();
  if (!row_live || !list || M_rows <= 0 || ((uintptr_t)list & 31)) return IA_ERR_ARG;
  hipLaunchKernelGGL(row_blocks_kernel, dim3(1), dim3(64), 0, stream, row_live, M_rows, (M_rows + 31) / 32, list, 0);
  return ia_check_launch();
}
static int row_blocks_host(const uint8_t* row_live, int M_rows, int* list, int gshift) {
  if (!row_live || !list || M_rows <= 0) return IA_ERR_ARG;
  const int nb = (M_rows + 31) / 32, nbr = (nb + 7) & ~7;
  int* const live = list + t256w::ROW_BLK_HDR;
  int* const dead = live + nbr;
  int n_live = 0;
  for (int t = 0; t < nb; ++t) {
    if (row_block_live(row_live, M_rows, t, gshift)) live[n_live++] = t; else dead[t - n_live] = t;
  }
  for (int i = 0; i < t256w::ROW_BLK_HDR; ++i) list[i] = 0;
  list[0] = n_live; list[1] = nb - n_live; list[2] = nb;
  return IA_OK;
}
extern "C" int ia_row_blocks_host(const uint8_t* row_live, int M_rows, int* list) { return row_blocks_host(row_live, M_rows, list, 0); }
// The group-aligned list (ABI 20): the layout of ia_row_blocks, the unit of liveness a 128-row group -- every block of a group that holds a
// live row is listed (in order, so entries 4i .. 4i+3 are one group; only the last group of M may have fewer), the blocks of the other
// groups are the dead list.
extern "C" size_t ia_row_groups_bytes(int M_rows) { return ia_row_blocks_bytes(M_rows); }
extern "C" int ia_row_groups(const uint8_t* row_live, int M_rows, int* list, hipStream_t stream) {
  (void)hipGetLastError();
  if (!row_live || !list || M_rows <= 0 || ((uintptr_t)list & 31)) return IA_ERR_ARG;
  hipLaunchKernelGGL(row_blocks_kernel, dim3(1), dim3(64), 0, stream, row_live, M_rows, (M_rows + 31) / 32, list, 2);
  return ia_check_launch();
}
extern "C" int ia_row_groups_host(const uint8_t* row_live, int M_rows, int* list) { return row_blocks_host(row_live, M_rows, list, 2); }
// ---- The slab list (EPI_SLABS): slab t = rows 8t .. 8t+7 (clipped to M), live = any row_live set.  Header: [0] live slabs, [1] dead slabs,
// [2] slabs.  The live slabs follow, ascending, 32 to an M-tile and inside a tile in the order [wave][piece] (the i-th live slab sits at
// slab_slot(i)); the entries behind the last one of the last tile are -1.  The dead slabs, ascending, start behind room for every slab
// rounded up to whole tiles.
static __host__ __device__ inline int slab_slot(int i) { return (i & ~31) + (i & 3) * 8 + ((i & 31) >> 2); }
static __host__ __device__ inline bool row_slab_live(const uint8_t* row_live, int M, int t) {
  const uint8_t* r = row_live + (size_t)t * 8;
  const int n = M - t * 8 < 8 ? M - t * 8 : 8;
  if (n == 8 && ((uintptr_t)r & 7) == 0) return *reinterpret_cast<const uint64_t*>(r) != 0;
  uint8_t any = 0;
  for (int i = 0; i < n; ++i) any |= r[i];
  return any != 0;
}
namespace {
// One wave, no LDS (row_blocks_kernel): lane l looks at slabs 64i + l.
__global__ __launch_bounds__(64) void row_slabs_kernel(const uint8_t* __restrict__ row_live, int M, int ns, int* __restrict__ out) {
  const int nsr = (ns + 31) & ~31;
  int* const live = out + t256w::ROW_BLK_HDR;
  int* const dead = live + nsr;
  const int lane = threadIdx.x;
  int base = 0;
  for (int c0 = 0; c0 < ns; c0 += 64 * 64) {
    uint64_t flags = 0;
#pragma unroll 8
    for (int i = 0; i < 64; ++i) {
      const int t = c0 + i * 64 + lane;
      if (t < ns && row_slab_live(row_live, M, t)) flags |= 1ull << i;
    }
    for (int i = 0; i < 64 && c0 + i * 64 < ns; ++i) {
      const int t = c0 + i * 64 + lane;
      const bool lv = (flags >> i) & 1ull;
      const uint64_t b = __ballot(lv);
      const int at = base + __popcll(b & ((1ull << lane) - 1ull));
      if (t < ns) { if (lv) live[slab_slot(at)] = t; else dead[t - at] = t; }
      base += __popcll(b);
    }
  }
  if (base + lane < ((base + 31) & ~31)) live[slab_slot(base + lane)] = -1;      // (at most 31 entries: the tail of the last tile)
  if (lane < t256w::ROW_BLK_HDR) out[lane] = lane == 0 ? base : (lane == 1 ? ns - base : (lane == 2 ? ns : 0));
}
}  // namespace
extern "C" size_t ia_row_slabs_bytes(int M_rows) {
  if (M_rows <= 0) return 0;
  const size_t nsr = (size_t)(((M_rows + 7) / 8 + 31) & ~31);
  return (t256w::ROW_BLK_HDR + 2 * nsr) * sizeof(int);
}
extern "C" int ia_row_slabs(const uint8_t* row_live, int M_rows, int* list, hipStream_t stream) {
  (void)hipGetLastError();
  if (!row_live || !list || M_rows <= 0 || ((uintptr_t)list & 31)) return IA_ERR_ARG;
  hipLaunchKernelGGL(row_slabs_kernel, dim3(1), dim3(64), 0, stream, row_live, M_rows, (M_rows + 7) / 8, list);
  return ia_check_launch();
}
extern "C" int ia_row_slabs_host(const uint8_t* row_live, int M_rows, int* list) {
  if (!row_live || !list || M_rows <= 0) return IA_ERR_ARG;
  const int ns = (M_rows + 7) / 8, nsr = (ns + 31) & ~31;
  int* const live = list + t256w::ROW_BLK_HDR;
  int* const dead = live + nsr;
  int n_live = 0;
  for (int t = 0; t < ns; ++t) {
    if (row_slab_live(row_live, M_rows, t)) live[slab_slot(n_live++)] = t; else dead[t - n_live] = t;
  }
  for (int i = n_live; i < ((n_live + 31) & ~31); ++i) live[slab_slot(i)] = -1;
  for (int i = 0; i < t256w::ROW_BLK_HDR; ++i) list[i] = 0;
  list[0] = n_live; list[1] = ns - n_live; list[2] = ns;
  return IA_OK;
}
// ---- The block-packed list (GemmArgs::rows_grouped == 2): the layout of ia_row_blocks -- header, slots, dead blocks -- with four slots per
// wave-row of the remapped kernel (eight per M-tile).  A wave-row holds the live 32-row blocks of one or more WHOLE 128-row groups: a group's
// blocks are contiguous and ascending, no group spans two wave-rows, the slots behind the last group are -1.  Header: [0] slots in use
// (4 x wave-rows), [1] dead blocks, [2] blocks.  Groups are placed by their number of live blocks (class) and their rank inside the class
// (ascending group index), a closed form of the class counts, so the device builder and its host twin agree by construction:
//   4 alone | each 3 with a 1 | 2 + 2 | an odd 2 left over with up to two 1s | the remaining 1s by four
// (705-733 wave-rows on masks like the benchmark's 512 x 255 rows against ceil(live blocks / 4) = 683-700 and 946-952 whole live groups).
// The last group when M cuts it short (M no multiple of 128) stays out of the classes and takes a wave-row of its own behind the others:
// the dense kernel runs that group through its guarded epilogue, whose column sums round differently (epi_store8), and so must the remap.
struct PackCounts { int n4, n3, n2, n1; };
static __host__ __device__ inline int pack_left1(const PackCounts& n) { return n.n1 > n.n3 ? n.n1 - n.n3 : 0; }      // 1s not paired with a 3
static __host__ __device__ inline int pack_take2(const PackCounts& n) { const int l = pack_left1(n); return (n.n2 & 1) ? (l < 2 ? l : 2) : 0; }
static __host__ __device__ inline int pack_rows(const PackCounts& n) {
  return n.n4 + n.n3 + ((n.n2 + 1) >> 1) + ((pack_left1(n) - pack_take2(n) + 3) >> 2);
}
// group of class c (1 .. 4 live blocks), rank r in its class -> first slot, and how many -1 slots it writes behind its blocks
static __host__ __device__ inline void pack_place(const PackCounts& n, int c, int r, int& slot, int& pad) {
  const int base2 = n.n4 + n.n3, base1 = base2 + ((n.n2 + 1) >> 1), take2 = pack_take2(n);
  pad = 0;
  if (c == 4) slot = 4 * r;
  else if (c == 3) { slot = 4 * (n.n4 + r); pad = r < n.n1 ? 0 : 1; }
  else if (c == 2) { slot = 4 * (base2 + (r >> 1)) + 2 * (r & 1); pad = ((n.n2 & 1) && r == n.n2 - 1 && take2 == 0) ? 2 : 0; }
  else if (r < n.n3) slot = 4 * (n.n4 + r) + 3;
  else if (r - n.n3 < take2) { slot = 4 * (base2 + (n.n2 >> 1)) + 2 + (r - n.n3); pad = (r - n.n3 == take2 - 1) ? 2 - take2 : 0; }
  else {
    const int q = r - n.n3 - take2;
    slot = 4 * base1 + q;
    pad = r == n.n1 - 1 ? 3 - (q & 3) : 0;
  }
}
namespace {
constexpr int PACK_MAX_GROUPS = 64 * 64;      // one wave, at most 64 rounds of 64 groups (M <= 524 288 rows)
// One wave, no LDS (see row_blocks_kernel).  Lane l owns groups 64 i + l: the four block flags of up to 64 groups sit in four 64-bit words
// per lane, a first pass of ballots counts the classes, a second one ranks every group in its class and among the dead blocks; each lane
// then writes its groups' slots (every slot exactly once: no fill pass) and dead-list entries.
__global__ __launch_bounds__(64) void row_groups_packed_kernel(const uint8_t* __restrict__ row_live, int M, int nb, int* __restrict__ out) {
  const int nbr = (nb + 7) & ~7, ngrp = (nb + 3) >> 2;
  int* const live = out + t256w::ROW_BLK_HDR;
  int* const dead = live + nbr;
  const int lane = threadIdx.x;
  const uint64_t lt = (1ull << lane) - 1ull;
  uint64_t f[4] = {0, 0, 0, 0};
  for (int i = 0; i * 64 < ngrp; ++i) {
    const int g = i * 64 + lane;
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (g < ngrp && 4 * g + j < nb && row_block_live(row_live, M, 4 * g + j)) f[j] |= 1ull << i;
  }
  auto cls = [&](int i) { return (int)((f[0] >> i) & 1ull) + (int)((f[1] >> i) & 1ull) + (int)((f[2] >> i) & 1ull) + (int)((f[3] >> i) & 1ull); };
  const int cut = (M & 127) ? ngrp - 1 : -1;     // the group M cuts short: outside the classes, a wave-row of its own at the end
  int cnt[5] = {0, 0, 0, 0, 0}, cut_rows = 0;
  for (int i = 0; i * 64 < ngrp; ++i) {
    const bool is_cut = i * 64 + lane == cut;
    const int c = is_cut ? 0 : cls(i);
#pragma unroll
    for (int k = 1; k <= 4; ++k) cnt[k] += __popcll(__ballot(c == k));
    cut_rows += __ballot(is_cut && cls(i) > 0) ? 1 : 0;
  }
  const PackCounts n{cnt[4], cnt[3], cnt[2], cnt[1]};
  int rank[5] = {0, 0, 0, 0, 0}, dbase = 0;
  for (int i = 0; i * 64 < ngrp; ++i) {
    const int g = i * 64 + lane, c_all = cls(i), c = g == cut ? 0 : c_all;
    int nblk = g < ngrp ? nb - 4 * g : 0;
    nblk = nblk > 4 ? 4 : nblk;
    const int nd = nblk - c_all;                 // dead blocks of this group
    int r = 0, dpos = dbase;
#pragma unroll
    for (int k = 1; k <= 4; ++k) {
      const uint64_t b = __ballot(c == k), d = __ballot(nd >= k);
      if (c == k) r = rank[k] + __popcll(b & lt);
      rank[k] += __popcll(b);
      dpos += __popcll(d & lt);
      dbase += __popcll(d);
    }
    if (g < ngrp) {
      if (c_all > 0) {
        int slot, pad;
        if (g == cut) { slot = 4 * pack_rows(n); pad = 4 - c_all; }
        else pack_place(n, c, r, slot, pad);
#pragma unroll
        for (int j = 0; j < 4; ++j)
          if ((f[j] >> i) & 1ull) live[slot++] = 4 * g + j;
        for (int k = 0; k < pad; ++k) live[slot++] = -1;
      }
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (j < nblk && !((f[j] >> i) & 1ull)) dead[dpos++] = 4 * g + j;
    }
  }
  if (lane < t256w::ROW_BLK_HDR) out[lane] = lane == 0 ? 4 * (pack_rows(n) + cut_rows) : (lane == 1 ? dbase : (lane == 2 ? nb : 0));
}
}  // namespace
extern "C" size_t ia_row_groups_packed_bytes(int M_rows) { return ia_row_blocks_bytes(M_rows); }
extern "C" int ia_row_groups_packed(const uint8_t* row_live, int M_rows, int* list, hipStream_t stream) {
  (void)hipGetLastError();
  if (!row_live || !list || M_rows <= 0 || ((uintptr_t)list & 31)) return IA_ERR_ARG;
  if ((M_rows + 127) / 128 > PACK_MAX_GROUPS) return IA_ERR_UNSUPPORTED;
  hipLaunchKernelGGL(row_groups_packed_kernel, dim3(1), dim3(64), 0, stream, row_live, M_rows, (M_rows + 31) / 32, list);
  return ia_check_launch();
}
extern "C" int ia_row_groups_packed_host(const uint8_t* row_live, int M_rows, int* list) {
  if (!row_live || !list || M_rows <= 0) return IA_ERR_ARG;
  if ((M_rows + 127) / 128 > PACK_MAX_GROUPS) return IA_ERR_UNSUPPORTED;
  const int nb = (M_rows + 31) / 32, nbr = (nb + 7) & ~7, ngrp = (nb + 3) >> 2;
  int* const live = list + t256w::ROW_BLK_HDR;
  int* const dead = live + nbr;
  PackCounts n{0, 0, 0, 0};
  auto cls = [&](int g) {
    int c = 0;
    for (int j = 0; j < 4 && 4 * g + j < nb; ++j) c += row_block_live(row_live, M_rows, 4 * g + j) ? 1 : 0;
    return c;
  };
  const int cut = (M_rows & 127) ? ngrp - 1 : -1;      // the group M cuts short: a wave-row of its own at the end
  for (int g = 0; g < ngrp; ++g) {
    const int c = g == cut ? 0 : cls(g);
    if (c == 4) ++n.n4; else if (c == 3) ++n.n3; else if (c == 2) ++n.n2; else if (c == 1) ++n.n1;
  }
  int rank[5] = {0, 0, 0, 0, 0}, n_dead = 0, cut_rows = 0;
  for (int g = 0; g < ngrp; ++g) {
    const int c = cls(g);
    int slot = 0, pad = 0;
    if (g == cut && c > 0) { slot = 4 * pack_rows(n); pad = 4 - c; cut_rows = 1; }
    else if (c > 0) pack_place(n, c, rank[c]++, slot, pad);
    for (int j = 0; j < 4 && 4 * g + j < nb; ++j) {
      if (row_block_live(row_live, M_rows, 4 * g + j)) live[slot++] = 4 * g + j; else dead[n_dead++] = 4 * g + j;
    }
    for (int k = 0; k < pad; ++k) live[slot++] = -1;
  }
  for (int i = 0; i < t256w::ROW_BLK_HDR; ++i) list[i] = 0;
  list[0] = 4 * (pack_rows(n) + cut_rows); list[1] = n_dead; list[2] = nb;
  return IA_OK;
}
// ---- the liveness mask of the weight gradient
// bit t of the mask = OR of row_live over rows 32 t .. 32 t + 31 (clipped to M): the 32-row blocks of k (ia_kblock_mask).  One function
// for the device kernel and the host entry.
template <int ROWS>
static __host__ __device__ inline uint32_t rows_live(const uint8_t* row_live, int M, int t) {
  const uint8_t* r = row_live + (size_t)t * ROWS;
  const int n = M - t * ROWS < ROWS ? M - t * ROWS : ROWS;
  uint64_t any = 0;
  if (n == ROWS && ((uintptr_t)r & 7) == 0) {
    for (int i = 0; i < ROWS / 8; ++i) any |= reinterpret_cast<const uint64_t*>(r)[i];
  } else {
    for (int i = 0; i < n; ++i) any |= r[i];
  }
  return any != 0 ? 1u : 0u;
}
namespace {
// one thread per bit, one 64-bit ballot per wave = two whole mask words, stored by lanes 0 and 32 (plain stores, no atomics)
__global__ __launch_bounds__(256) void kblock_mask_kernel(const uint8_t* __restrict__ row_live, int M, int nb, uint32_t* __restrict__ mask) {
  const int b = blockIdx.x * 256 + threadIdx.x;
  const uint64_t v = __ballot(b < nb && rows_live<32>(row_live, M, b));
  if ((threadIdx.x & 31) == 0 && b < nb) mask[b >> 5] = (uint32_t)(v >> (threadIdx.x & 32));
}
}  // namespace
extern "C" size_t ia_kblock_mask_bytes(int M_rows) { return M_rows <= 0 ? 0 : (size_t)(((M_rows + 31) / 32 + 31) / 32) * sizeof(uint32_t); }
extern "C" int ia_kblock_mask(const uint8_t* row_live, int M_rows, uint32_t* mask, hipStream_t stream) {
  (void)hipGetLastError();
  if (!row_live || !mask || M_rows <= 0) return IA_ERR_ARG;
  const int nb = (M_rows + 31) / 32;
  hipLaunchKernelGGL(kblock_mask_kernel, dim3((nb + 255) / 256), dim3(256), 0, stream, row_live, M_rows, nb, mask);
  return ia_check_launch();
}
extern "C" int ia_kblock_mask_host(const uint8_t* row_live, int M_rows, uint32_t* mask) {
  if (!row_live || !mask || M_rows <= 0) return IA_ERR_ARG;
  const int nb = (M_rows + 31) / 32;
  for (int w = 0; w < (nb + 31) / 32; ++w) mask[w] = 0u;
  for (int t = 0; t < nb; ++t) mask[t >> 5] |= rows_live<32>(row_live, M_rows, t) << (t & 31);
  return IA_OK;
}
// ... and of its walk over 16-row steps: bit s = OR of row_live over rows 16 s .. 16 s + 15 (clipped to M) (ia_kstep_mask).  The same
// per-bit function, the same launch shape.
namespace {
__global__ __launch_bounds__(256) void kstep_mask_kernel(const uint8_t* __restrict__ row_live, int M, int ns, uint32_t* __restrict__ mask) {
  const int b = blockIdx.x * 256 + threadIdx.x;
  const uint64_t v = __ballot(b < ns && rows_live<16>(row_live, M, b));
  if ((threadIdx.x & 31) == 0 && b < ns) mask[b >> 5] = (uint32_t)(v >> (threadIdx.x & 32));
}
// the block mask of a step mask (block t = steps 2t and 2t + 1), for a launch whose k-slab is too long for the step walk: one thread per
// block bit, the same ballot and plain stores
__global__ __launch_bounds__(256) void kblock_of_ksteps_kernel(const uint32_t* __restrict__ steps, int ns, int nb, uint32_t* __restrict__ mask) {
  const int b = blockIdx.x * 256 + threadIdx.x;
  bool live = false;
  if (b < nb) {
    const uint32_t w = steps[(2 * b) >> 5] >> ((2 * b) & 31);      // (steps 2b and 2b + 1 share a word; a step behind ns has a zero bit)
    live = (w & (2 * b + 1 < ns ? 3u : 1u)) != 0u;
  }
  const uint64_t v = __ballot(live);
  if ((threadIdx.x & 31) == 0 && b < nb) mask[b >> 5] = (uint32_t)(v >> (threadIdx.x & 32));
}
}  // namespace
extern "C" size_t ia_kstep_mask_bytes(int M_rows) { return M_rows <= 0 ? 0 : (size_t)(((M_rows + 15) / 16 + 31) / 32) * sizeof(uint32_t); }
extern "C" int ia_kstep_mask(const uint8_t* row_live, int M_rows, uint32_t* mask, hipStream_t stream) {
  (void)hipGetLastError();
  if (!row_live || !mask || M_rows <= 0) return IA_ERR_ARG;
  const int ns = (M_rows + 15) / 16;
  hipLaunchKernelGGL(kstep_mask_kernel, dim3((ns + 255) / 256), dim3(256), 0, stream, row_live, M_rows, ns, mask);
  return ia_check_launch();
}
extern "C" int ia_kstep_mask_host(const uint8_t* row_live, int M_rows, uint32_t* mask) {
  if (!row_live || !mask || M_rows <= 0) return IA_ERR_ARG;
  const int ns = (M_rows + 15) / 16;
  for (int w = 0; w < (ns + 31) / 32; ++w) mask[w] = 0u;
  for (int t = 0; t < ns; ++t) mask[t >> 5] |= rows_live<16>(row_live, M_rows, t) << (t & 31);
  return IA_OK;
}

// ---- one descriptor for all of them (IaRowFilter, common.h): the list of a kind, by size and by builder
size_t ia_row_filter_bytes(IaRowFilter::Kind kind, int M) {
  switch (kind) {
    case IaRowFilter::BLOCKS: return ia_row_blocks_bytes(M);
    case IaRowFilter::GROUPS: return ia_row_groups_bytes(M);
    case IaRowFilter::PACKED: return ia_row_groups_packed_bytes(M);
    case IaRowFilter::SLABS: return ia_row_slabs_bytes(M);
    case IaRowFilter::KBLOCKS: return ia_kblock_mask_bytes(M);
    case IaRowFilter::KSTEPS: return ia_kstep_mask_bytes(M);
    case IaRowFilter::NONE: break;
  }
  return 0;
}
int ia_row_filter_build(IaRowFilter::Kind kind, const uint8_t* row_live, int M, void* dst, hipStream_t stream) {
  switch (kind) {
    case IaRowFilter::BLOCKS: return ia_row_blocks(row_live, M, (int*)dst, stream);
    case IaRowFilter::GROUPS: return ia_row_groups(row_live, M, (int*)dst, stream);
    case IaRowFilter::PACKED: return ia_row_groups_packed(row_live, M, (int*)dst, stream);
    case IaRowFilter::SLABS: return ia_row_slabs(row_live, M, (int*)dst, stream);
    case IaRowFilter::KBLOCKS: return ia_kblock_mask(row_live, M, (uint32_t*)dst, stream);
    case IaRowFilter::KSTEPS: return ia_kstep_mask(row_live, M, (uint32_t*)dst, stream);
    case IaRowFilter::NONE: break;
  }
  return IA_ERR_ARG;
}

// ---- the filtered GEMMs.  Which (kind, epilogue) pairs have a kernel form is stated HERE, once per direction; every entry below asks.
bool ia_gemm_fwd_form(IaRowFilter::Kind kind, int e) {
  switch (kind) {
    case IaRowFilter::NONE: return true;
    case IaRowFilter::BLOCKS: return e == EPI_NONE || e == EPI_BIAS || e == EPI_BIAS_GELU || e == EPI_BIAS_GELU_ACT || e == EPI_BIAS_ADD;
    case IaRowFilter::SLABS: return e == EPI_NONE || e == EPI_BIAS || e == EPI_BIAS_GELU;
    default: return false;
  }
}
bool ia_gemm_dgrad_form(IaRowFilter::Kind kind, int e) {
  switch (kind) {
    case IaRowFilter::NONE: return true;
    case IaRowFilter::BLOCKS: return e == EPI_NONE || e == EPI_ADD || e == EPI_DGELU_CS;
    // the column sums keep the dense kernel's partials: whole 128-row groups, or the live blocks packed by whole groups
    case IaRowFilter::GROUPS: case IaRowFilter::PACKED: return e == EPI_DGELU_CS;
    case IaRowFilter::SLABS: return e == EPI_NONE || e == EPI_ADD;
    default: return false;
  }
}
int ia_gemm_fwd_filtered(const void* X, int ldx, const void* W, int ldw, void* Y, int ldy, int M_rows, int N_out, int K_in, int epilogue,
                         const float* bias, const void* aux, int ldaux, void* C2, int scaled_cols, float col_scale, IaRowFilter filter,
                         hipStream_t stream) {
  if (!ia_gemm_fwd_form(filter.kind, epilogue)) return IA_ERR_UNSUPPORTED;
  GemmCall c{X, 0, ldx, W, 0, ldw, Y, 0, ldy, M_rows, N_out, K_in};
  c.epilogue = epilogue; c.bias = bias; c.aux = aux; c.ldaux = ldaux; c.C2 = C2; c.qcols = scaled_cols; c.qscale = col_scale; c.filter = filter;
  return gemm_core(c, stream);
}
int ia_gemm_dgrad_filtered(const void* dY, int ldy, const void* W, int w_kstrided, int ldw, void* dX, int ldx, int M_rows, int N_in, int K_out,
                           int epilogue, const void* aux, int ldaux, void* C2, IaRowFilter filter, void* workspace, size_t workspace_bytes,
                           hipStream_t stream) {
  if (!ia_gemm_dgrad_form(filter.kind, epilogue)) return IA_ERR_UNSUPPORTED;
  GemmCall c{dY, 0, ldy, W, w_kstrided, ldw, dX, 0, ldx, M_rows, N_in, K_out};
  c.epilogue = epilogue; c.aux = aux; c.ldaux = ldaux; c.C2 = C2; c.workspace = workspace; c.workspace_bytes = workspace_bytes;
  c.filter = filter; c.filter.fill = true;      // not every consumer of a data gradient filters its rows
  return gemm_core(c, stream);
}
extern "C" int ia_gemm_wgrad_walk(int N_out, int N_in, int M_rows);
int ia_gemm_wgrad_filtered(const void* dY, int ldy, const void* X, int ldx, float* dW, int ldw, int N_out, int N_in, int M_rows, IaRowFilter filter,
                           int accumulate, void* workspace, size_t workspace_bytes, hipStream_t stream) {
  if (filter.kind != IaRowFilter::NONE && filter.kind != IaRowFilter::KBLOCKS && filter.kind != IaRowFilter::KSTEPS) return IA_ERR_UNSUPPORTED;
  // A step mask on a shape whose k-slab is too long for the step walk (ia_gemm_wgrad_walk says 1): the block walk, from the block mask
  // of the step mask, built behind the split-K partials where the workspace has the room ia_gemm_wgrad_rows_workspace_bytes asks for
  // (one small launch); without that room, every row.
  if (filter.kind == IaRowFilter::KSTEPS && filter.list && ia_gemm_wgrad_walk(N_out, N_in, M_rows) == 1) {
    const size_t front = al256(ia_gemm_workspace_bytes(N_out, N_in, M_rows, 1));
    const uint32_t* const steps = (const uint32_t*)filter.list;
    filter = IaRowFilter{};
    if (workspace && workspace_bytes >= front + ia_kblock_mask_bytes(M_rows)) {
      uint32_t* const bm = (uint32_t*)((char*)workspace + front);
      const int ns = (M_rows + 15) / 16, nb = (M_rows + 31) / 32;
      (void)hipGetLastError();
      hipLaunchKernelGGL(kblock_of_ksteps_kernel, dim3((nb + 255) / 256), dim3(256), 0, stream, steps, ns, nb, bm);
      int rc = ia_check_launch();
      if (rc) return rc;
      filter = IaRowFilter{IaRowFilter::KBLOCKS, bm};
      workspace_bytes = front;
    }
  }
  GemmCall c{dY, 1, ldy, X, 1, ldx, dW, 1, ldw, N_out, N_in, M_rows};
  c.accumulate = accumulate; c.workspace = workspace; c.workspace_bytes = workspace_bytes; c.filter = filter;
  return gemm_core(c, stream);
}
// The x gelu' + column-sums data gradient over a block-packed list: dX = (dY W) * aux on the live 32-row blocks, the other rows as zeros, and
// C2 += the column sums, bit-identical to ia_gemm_bf16's (IA_EPI_DGELU_COLSUM) on a dY whose rows are zero wherever the list has no block.
// A shape the remapped kernel does not serve runs every row.
extern "C" int ia_gemm_dgrad_packed(const void* dY, int ldy, const void* W, int w_kstrided, int ldw, void* dX, int ldx, int M_rows, int N_in, int K_out,
                                    const void* aux, int ldaux, void* C2, const int* packed_list, void* workspace, size_t workspace_bytes,
                                    hipStream_t stream) {
  return ia_gemm_dgrad_filtered(dY, ldy, W, w_kstrided, ldw, dX, ldx, M_rows, N_in, K_out, EPI_DGELU_CS, aux, ldaux, C2,
                                IaRowFilter{IaRowFilter::PACKED, packed_list}, workspace, workspace_bytes, stream);
}
// the weight gradient over the live 32-row blocks of a prebuilt ia_kblock_mask (NULL: every row)
extern "C" int ia_gemm_wgrad_blocks(const void* dY, int ldy, const void* X, int ldx, float* dW, int ldw, int N_out, int N_in, int M_rows,
                                    const uint32_t* kblock_mask, int accumulate, void* workspace, size_t workspace_bytes, hipStream_t stream) {
  return ia_gemm_wgrad_filtered(dY, ldy, X, ldx, dW, ldw, N_out, N_in, M_rows, IaRowFilter{IaRowFilter::KBLOCKS, kblock_mask}, accumulate, workspace,
                                workspace_bytes, stream);
}

// ... and over the live 16-row steps of a prebuilt ia_kstep_mask (NULL: every row), four to a k-tile.  Bit-identical to the call above on
// the same rows.  A shape whose k-slabs are too long for the step walk (ia_gemm_wgrad_walk) takes the block walk.
extern "C" int ia_gemm_wgrad_steps(const void* dY, int ldy, const void* X, int ldx, float* dW, int ldw, int N_out, int N_in, int M_rows,
                                   const uint32_t* kstep_mask, int accumulate, void* workspace, size_t workspace_bytes, hipStream_t stream) {
  return ia_gemm_wgrad_filtered(dY, ldy, X, ldx, dW, ldw, N_out, N_in, M_rows, IaRowFilter{IaRowFilter::KSTEPS, kstep_mask}, accumulate, workspace,
                                workspace_bytes, stream);
}

// ---- the public entries that take the rows' live bytes: build the list in the workspace, then the filtered call
// What the seven share (rows: the token rows, n1 / n2: the GEMM's other two sizes).  Without row_live: a filter with no list (every row; the
// GEMM keeps the caller's whole workspace).  With it: the shape is checked, the list of `kind` is carved behind the first `front` bytes of the workspace (the GEMM's own part: column-sum or
// split-K partials) and built, and *workspace_bytes leaves as `front`.  The workspace is 32-byte aligned for a list, 16 for a mask.
static int filter_from_rows(IaRowFilter::Kind kind, const uint8_t* row_live, int fill, int rows, int n1, int n2, size_t front, void* workspace,
                            size_t* workspace_bytes, hipStream_t stream, IaRowFilter* filter) {
  *filter = IaRowFilter{kind, nullptr, fill != 0};
  if (!row_live) return IA_OK;
  if (rows <= 0 || n1 <= 0 || n2 <= 0) return IA_ERR_ARG;
  const uintptr_t align = kind == IaRowFilter::KBLOCKS ? 15 : 31;
  if (!workspace || *workspace_bytes < front + ia_row_filter_bytes(kind, rows) || ((uintptr_t)workspace & align)) return IA_ERR_WORKSPACE;
  void* const list = (char*)workspace + front;
  filter->list = list;
  *workspace_bytes = front;
  return ia_row_filter_build(kind, row_live, rows, list, stream);
}
extern "C" size_t ia_gemm_fwd_rows_workspace_bytes(int M_rows) { return ia_row_blocks_bytes(M_rows); }
extern "C" size_t ia_gemm_slabs_workspace_bytes(int M_rows) { return ia_row_slabs_bytes(M_rows); }
// 1: a call of this shape (rows contiguous: ldx = K_in, ldy = N_out) with row_live computes the live 32-row blocks only; 0: every row
extern "C" int ia_gemm_fwd_rows_filters(int M_rows, int N_out, int K_in) {
  if (M_rows <= 0 || N_out <= 0 || K_in <= 0 || (K_in & 7) || (N_out & 7)) return 0;
  return make_plan(M_rows, N_out, K_in, false).big && dgrad_rows_fit(M_rows, K_in, N_out, 0) ? 1 : 0;
}
// ia_gemm_fwd_rows (32-row blocks) and ia_gemm_fwd_slabs (8-row slabs)
static int gemm_fwd_rows(IaRowFilter::Kind kind, const void* X, int ldx, const void* W, int ldw, void* Y, int ldy, int M_rows, int N_out, int K_in,
                         int epilogue, const float* bias, void* C2, int scaled_cols, float col_scale, const uint8_t* row_live, int fill_dead_rows,
                         void* workspace, size_t workspace_bytes, hipStream_t stream) {
  // (IA_EPI_BIAS_ADD needs an aux these two have no argument for: ia_gemm_fwd_rows_add)
  if (epilogue == EPI_BIAS_ADD || !ia_gemm_fwd_form(kind, epilogue)) return IA_ERR_UNSUPPORTED;
  IaRowFilter f;
  int rc = filter_from_rows(kind, row_live, fill_dead_rows, M_rows, N_out, K_in, 0, workspace, &workspace_bytes, stream, &f);
  return rc ? rc : ia_gemm_fwd_filtered(X, ldx, W, ldw, Y, ldy, M_rows, N_out, K_in, epilogue, bias, nullptr, 0, C2, scaled_cols, col_scale, f, stream);
}
extern "C" int ia_gemm_fwd_rows(const void* X, int ldx, const void* W, int ldw, void* Y, int ldy, int M_rows, int N_out, int K_in, int epilogue,
                                const float* bias, void* C2, int scaled_cols, float col_scale, const uint8_t* row_live, int fill_dead_rows,
                                void* workspace, size_t workspace_bytes, hipStream_t stream) {
  return gemm_fwd_rows(IaRowFilter::BLOCKS, X, ldx, W, ldw, Y, ldy, M_rows, N_out, K_in, epilogue, bias, C2, scaled_cols, col_scale, row_live,
                       fill_dead_rows, workspace, workspace_bytes, stream);
}
extern "C" int ia_gemm_fwd_slabs(const void* X, int ldx, const void* W, int ldw, void* Y, int ldy, int M_rows, int N_out, int K_in, int epilogue,
                                 const float* bias, void* C2, int scaled_cols, float col_scale, const uint8_t* row_live, int fill_dead_rows,
                                 void* workspace, size_t workspace_bytes, hipStream_t stream) {
  return gemm_fwd_rows(IaRowFilter::SLABS, X, ldx, W, ldw, Y, ldy, M_rows, N_out, K_in, epilogue, bias, C2, scaled_cols, col_scale, row_live,
                       fill_dead_rows, workspace, workspace_bytes, stream);
}
// Y = X W^T + bias + aux over the live 32-row blocks (the fc2 of a pre-LN layer, bias + residual)
extern "C" int ia_gemm_fwd_rows_add(const void* X, int ldx, const void* W, int ldw, void* Y, int ldy, int M_rows, int N_out, int K_in,
                                    const float* bias, const void* aux, int ldaux, const uint8_t* row_live, int fill_dead_rows, void* workspace,
                                    size_t workspace_bytes, hipStream_t stream) {
  IaRowFilter f;
  int rc = filter_from_rows(IaRowFilter::BLOCKS, row_live, fill_dead_rows, M_rows, N_out, K_in, 0, workspace, &workspace_bytes, stream, &f);
  return rc ? rc : ia_gemm_fwd_filtered(X, ldx, W, ldw, Y, ldy, M_rows, N_out, K_in, EPI_BIAS_ADD, bias, aux, ldaux, nullptr, 0, 1.f, f, stream);
}
extern "C" size_t ia_gemm_dgrad_rows_workspace_bytes(int M_rows, int N_in, int K_out) {
  if (M_rows <= 0 || N_in <= 0 || K_out <= 0) return 0;
  return al256(ia_gemm_colsum_workspace_bytes(M_rows, N_in)) + ia_row_blocks_bytes(M_rows);
}
// 1: a call of this shape (rows contiguous: ldy = K_out, ldx = ldaux = N_in) with row_live computes the live 32-row blocks only; 0: it
// runs every row, like ia_gemm_bf16 (the same conditions as gemm_core's)
extern "C" int ia_gemm_dgrad_rows_filters(int M_rows, int N_in, int K_out) {
  if (M_rows <= 0 || N_in <= 0 || K_out <= 0 || (K_out & 7)) return 0;
  return make_plan(M_rows, N_in, K_out, false).big && dgrad_rows_fit(M_rows, K_out, N_in, N_in) ? 1 : 0;
}
// ia_gemm_dgrad_rows (32-row blocks), ia_gemm_dgrad_groups_rows (128-row groups) and ia_gemm_dgrad_slabs (8-row slabs).  The two with
// column sums keep those partials in front of the workspace and the list behind them; the slab form has no workspace of the GEMM's own.
static int gemm_dgrad_rows(IaRowFilter::Kind kind, const void* dY, int ldy, const void* W, int w_kstrided, int ldw, void* dX, int ldx, int M_rows,
                           int N_in, int K_out, int epilogue, const void* aux, int ldaux, void* C2, const uint8_t* row_live, void* workspace,
                           size_t workspace_bytes, hipStream_t stream) {
  if (!ia_gemm_dgrad_form(kind, epilogue)) return IA_ERR_UNSUPPORTED;
  const size_t front = kind == IaRowFilter::SLABS ? 0 : al256(ia_gemm_colsum_workspace_bytes(M_rows, N_in));
  IaRowFilter f;
  int rc = filter_from_rows(kind, row_live, 1, M_rows, N_in, K_out, front, workspace, &workspace_bytes, stream, &f);
  return rc ? rc : ia_gemm_dgrad_filtered(dY, ldy, W, w_kstrided, ldw, dX, ldx, M_rows, N_in, K_out, epilogue, aux, ldaux, C2, f, workspace,
                                          workspace_bytes, stream);
}
extern "C" int ia_gemm_dgrad_rows(const void* dY, int ldy, const void* W, int w_kstrided, int ldw, void* dX, int ldx, int M_rows, int N_in,
                                  int K_out, int epilogue, const void* aux, int ldaux, void* C2, const uint8_t* row_live, void* workspace,
                                  size_t workspace_bytes, hipStream_t stream) {
  return gemm_dgrad_rows(IaRowFilter::BLOCKS, dY, ldy, W, w_kstrided, ldw, dX, ldx, M_rows, N_in, K_out, epilogue, aux, ldaux, C2, row_live, workspace,
                         workspace_bytes, stream);
}
extern "C" int ia_gemm_dgrad_groups_rows(const void* dY, int ldy, const void* W, int w_kstrided, int ldw, void* dX, int ldx, int M_rows, int N_in,
                                         int K_out, const void* aux, int ldaux, void* C2, const uint8_t* row_live, void* workspace,
                                         size_t workspace_bytes, hipStream_t stream) {
  return gemm_dgrad_rows(IaRowFilter::GROUPS, dY, ldy, W, w_kstrided, ldw, dX, ldx, M_rows, N_in, K_out, EPI_DGELU_CS, aux, ldaux, C2, row_live,
                         workspace, workspace_bytes, stream);
}
extern "C" int ia_gemm_dgrad_slabs(const void* dY, int ldy, const void* W, int w_kstrided, int ldw, void* dX, int ldx, int M_rows, int N_in,
                                   int K_out, int epilogue, const void* aux, int ldaux, const uint8_t* row_live, void* workspace,
                                   size_t workspace_bytes, hipStream_t stream) {
  return gemm_dgrad_rows(IaRowFilter::SLABS, dY, ldy, W, w_kstrided, ldw, dX, ldx, M_rows, N_in, K_out, epilogue, aux, ldaux, nullptr, row_live, workspace,
                         workspace_bytes, stream);
}
extern "C" size_t ia_gemm_wgrad_rows_workspace_bytes(int N_out, int N_in, int M_rows) {
  if (N_out <= 0 || N_in <= 0 || M_rows <= 0) return 0;
  return al256(ia_gemm_workspace_bytes(N_out, N_in, M_rows, 1)) + ia_kblock_mask_bytes(M_rows);
}
// 1: a call of this shape with row_live and the workspace of the query above walks the live 32-row blocks (256-wide kernel, a k-slab
// the mask words of one wave cover: t256w::blk_mask_fits); 0: it runs every row, like ia_gemm_bf16 (the same conditions as gemm_core's)
extern "C" int ia_gemm_wgrad_rows_filters(int N_out, int N_in, int M_rows) {
  if (N_out <= 0 || N_in <= 0 || M_rows <= 0) return 0;
  const Plan pl = make_plan(N_out, N_in, M_rows, true);
  const int nk = (M_rows + BK - 1) / BK;
  return pl.big && t256w::blk_mask_fits((nk + pl.splits - 1) / pl.splits) ? 1 : 0;
}
// which walk a filtered weight gradient of this shape takes: 2 = the live 16-row steps (given a step mask: ia_gemm_wgrad_steps, the engine),
// 1 = the live 32-row blocks (the k-slab is too long for the step walk's mask words, step_mask_fits), 0 = every row
extern "C" int ia_gemm_wgrad_walk(int N_out, int N_in, int M_rows) {
  if (N_out <= 0 || N_in <= 0 || M_rows <= 0) return 0;
  const Plan pl = make_plan(N_out, N_in, M_rows, true);
  const int nk = (M_rows + BK - 1) / BK, slab = (nk + pl.splits - 1) / pl.splits;
  if (!pl.big) return 0;
  return t256w::step_mask_fits(slab) ? 2 : (t256w::blk_mask_fits(slab) ? 1 : 0);
}
// the weight gradient over the live 32-row blocks: the split-K partials in front of the workspace, the mask behind them
extern "C" int ia_gemm_wgrad_rows(const void* dY, int ldy, const void* X, int ldx, float* dW, int ldw, int N_out, int N_in, int M_rows,
                                  const uint8_t* row_live, int accumulate, void* workspace, size_t workspace_bytes, hipStream_t stream) {
  IaRowFilter f;
  int rc = filter_from_rows(IaRowFilter::KBLOCKS, row_live, 1, M_rows, N_out, N_in, al256(ia_gemm_workspace_bytes(N_out, N_in, M_rows, 1)), workspace,
                            &workspace_bytes, stream, &f);
  return rc ? rc : ia_gemm_wgrad_filtered(dY, ldy, X, ldx, dW, ldw, N_out, N_in, M_rows, f, accumulate, workspace, workspace_bytes, stream);
}


// GEMM with shifted operand views and channel groups batched into one launch (see GemmArgs): the building block of the
// patch-matrix-free 3x3 convolution in conv.hip (library-internal, declared in common.h).
int ia_gemm_view(const IaViewGemm& v, hipStream_t stream) {
  if ((v.a_view && (v.a_kstrided || (v.a_view != 1 && v.a_view != -1))) || (v.b_view && (!v.b_kstrided || v.b_view < 1 || v.b_view > 2)) ||
      v.pw <= 2 || (!v.a_view && !v.b_view) || v.groups < 1 || v.lca < 3 || v.lcbk < 3 || v.lcbn < 3)
    return IA_ERR_ARG;
  GemmCall c{v.A, v.a_kstrided, v.lda, v.B, v.b_kstrided, v.ldb, v.C, v.c_is_f32, v.ldc, v.M, v.N, v.K};
  c.epilogue = v.bias ? EPI_BIAS : EPI_NONE; c.bias = v.bias; c.C2 = v.rsum_out; c.workspace = v.workspace; c.workspace_bytes = v.workspace_bytes;
  c.view = &v;
  return gemm_core(c, stream);
}

size_t ia_gemm_view_workspace_bytes(int M, int N, int K, int groups) {
  if (M <= 0 || N <= 0 || K <= 0 || groups <= 0) return 0;
  const Plan pl = make_plan(M, N, K, true, groups);
  return pl.splits > 1 ? (size_t)groups * pl.splits * M * (N + 1) * sizeof(float) : 0;      // + the row-sum partials (bias gradient)
}

// EPI_DGELU_CS (k-contiguous A, bf16 output): csum (fp32 [N]) += column sums of the output -- the bias gradient of the Linear in front
// of the GELU
template <bool BKS>
static int launch_dgelu_colsum(GemmArgs& g, bool big, float* csum, void* workspace, size_t workspace_bytes, hipStream_t stream) {
  if (!csum || !workspace || workspace_bytes < ia_gemm_colsum_workspace_bytes(g.M, g.N) || g.ldc != g.N) return IA_ERR_WORKSPACE;
  if (!big) {                                  // small shapes: plain epilogue, then the stand-alone column-sum kernel
    int rc = launch<false, BKS, EPI_DGELU, false>(g, false, stream);
    return rc ? rc : ia_colsum(g.C, g.ldc, g.M, g.N, csum, 1, workspace, workspace_bytes, stream);
  }
  g.csum_part = (float*)workspace;
  int rc = launch<false, BKS, EPI_DGELU_CS, false>(g, true, stream);
  return rc ? rc : ia_sum_rows_f32((const float*)workspace, ((g.M + 255) / 256) * 2, g.N, csum, 1, stream);
}

static int gemm_core(const GemmCall& c, hipStream_t stream) {
  const IaViewGemm* const view = c.view;
  const int M = c.M, N = c.N, K = c.K, epilogue = c.epilogue;
  const bool aks = c.a_kstrided != 0, bks = c.b_kstrided != 0, f32 = c.c_is_f32 != 0;
  const uint64_t a_window = view ? view->a_window : 0, b_window = view ? view->b_window : 0;
  const int groups = view ? view->groups : 1;
  (void)hipGetLastError();  // drop stale status left by unrelated runtime calls (e.g. hipEventQuery -> NotReady)
  if (!c.A || !c.B || !c.C || M <= 0 || N <= 0 || K <= 0) return IA_ERR_ARG;
  if ((c.lda & 7) || (c.ldb & 7) || (c.ldc & 3) || (N & 3)) return IA_ERR_ARG;
  if (((uintptr_t)c.A & 15) || ((uintptr_t)c.B & 15) || ((uintptr_t)c.C & 15)) return IA_ERR_ARG;
  GemmArgs g;
  g.A = (const bf16*)c.A; g.B = (const bf16*)c.B; g.C = c.C; g.C2 = (bf16*)c.C2; g.bias = c.bias; g.aux = (const bf16*)c.aux;
  g.M = M; g.N = N; g.K = K; g.lda = c.lda; g.ldb = c.ldb; g.ldc = c.ldc; g.ldaux = c.ldaux; g.accumulate = c.accumulate;
  if (c.qcols < 0 || c.qcols > N || (c.qcols & 127) || (c.qcols && (epilogue != EPI_BIAS || f32 || aks || bks))) return IA_ERR_ARG;
  g.qcols = c.qcols; g.qscale = c.qscale;
  // (k-strided A with an odd M: the buffer range check works on whole dwords, so a window that ends in the middle of one loses the last
  // element of the last k row -- C[M-1][*] came out without its k = K-1 product, the row sums without A[K-1][M-1].  The window ends behind
  // that dword instead: its other half lies inside the row's pitch (lda is a multiple of 8, so lda > M) and only feeds row M, which is
  // never stored.  Every other operand ends on a dword: K is a multiple of 8 where A is k-contiguous, N a multiple of 4.)
  const uint64_t ab = a_window ? a_window : (aks ? (((uint64_t)(K - 1) * c.lda + M) * 2 + 3) & ~(uint64_t)3 : ((uint64_t)(M - 1) * c.lda + K) * 2);
  const uint64_t bb = b_window ? b_window : (bks ? ((uint64_t)(K - 1) * c.ldb + N) * 2 : ((uint64_t)(N - 1) * c.ldb + K) * 2);
  g.csum_part = nullptr; g.split_id = 0; g.tile_ctr = nullptr;
  g.a_view = g.b_view = g.pw = 0; g.lca = g.lcbk = g.lcbn = 6;
  g.groups = 1; g.ga = g.gb = g.gc = g.gbias = 0;
  if (view) {
    g.a_view = view->a_view; g.b_view = view->b_view; g.pw = view->pw; g.lca = view->lca; g.lcbk = view->lcbk; g.lcbn = view->lcbn;
    g.groups = groups; g.ga = view->ga; g.gb = view->gb; g.gc = view->gc; g.gbias = view->gbias;
  }
  if (!aks && (K & 7)) return IA_ERR_ARG;
  g.a_bytes = ab; g.b_bytes = bb;
  g.tiles_m = g.tiles_n = 0;
  { static int dbg = -1; if (dbg < 0) { const char* e = getenv("IA_GEMM_DBG"); dbg = e ? atoi(e) : 0; } g.dbg = dbg; }
  const int nk = (K + BK - 1) / BK;
  Plan pl = make_plan(M, N, K, f32, groups);
  g.splits = 1; g.nk_per_split = nk; g.ws = nullptr;
  const bool big = pl.big && !view && !(g.dbg & 128);     // the shifted views and the group batching live in the T128 kernel only (dbg 128: force T128)
  // weight-gradient form with C2: the fp32 row sums of A^T (bias gradient) come out of the same launch (T128 kernel)
  const bool wgrad_form = aks && bks && f32 && epilogue == EPI_NONE;
  g.rsum_out = (wgrad_form && !big) ? (float*)c.C2 : nullptr;
  g.rsum_ws = nullptr;
  // split-K sums partial products: only the plain epilogue may be cut (a bias would be added once per k-slab -- the fp32 + bias form
  // came out with 2-8 x the bias until round 2's edge-shape test)
  if (f32 && epilogue == EPI_NONE && pl.splits > 1 && c.workspace &&
      c.workspace_bytes >= (size_t)groups * pl.splits * M * (N + (g.rsum_out ? 1 : 0)) * sizeof(float)) {
    g.nk_per_split = (nk + pl.splits - 1) / pl.splits;
    g.splits = (nk + g.nk_per_split - 1) / g.nk_per_split;
    g.ws = (float*)c.workspace;
    g.rsum_ws = g.ws + (size_t)groups * g.splits * M * N;
  }
  {  // every workgroup addresses its operands through a 32-bit buffer window that starts at its tile / k-slab (rsrc_at): that
     // window -- not the tensor -- has to stay below 2 GiB
    const uint64_t margin = view ? 2 * (uint64_t)(view->pw + 1) : 0, slab = (uint64_t)g.nk_per_split * BK + margin, tile = 256 + margin;
    const uint64_t wa = (aks ? slab : tile) * (uint64_t)c.lda * 2 + (aks ? 0 : (uint64_t)K * 2);
    const uint64_t wb = (bks ? slab : tile) * (uint64_t)c.ldb * 2 + (bks ? 0 : (uint64_t)K * 2);
    if (wa >= 0x7FFFFFF0ull || wb >= 0x7FFFFFF0ull) return IA_ERR_ARG;
  }
  // What the filter holds: a mask of the live k (weight gradient), or a list of the live rows (the other forms).  Which (kind, epilogue)
  // pairs exist is the business of ia_gemm_fwd_form / ia_gemm_dgrad_form; here a filter only ever falls back to every row.
  const IaRowFilter::Kind kind = c.filter.kind;
  const bool k_steps = kind == IaRowFilter::KSTEPS, k_mask = kind == IaRowFilter::KBLOCKS || k_steps, row_list = kind != IaRowFilter::NONE && !k_mask;
  // the live-block mask: the 256-wide weight-gradient kernel only, one mask word per lane and k-slab (anything else runs dense).
  // GemmArgs::live_blk shares the slot of GemmArgs::bias (filled above from the caller's argument): in the weight-gradient form, whose
  // 256-wide kernel reads the slot as the mask, it is overwritten HERE for every caller -- a stray bias passed with IA_EPI_NONE, the
  // shifted views of ia_gemm_view -- so the kernel sees a mask or NULL, never a bias.  launch<true, true, EPI_NONE, true> is reached
  // from this function only; a new call site that fills GemmArgs for this form must do the same.
  // (a step mask on a slab step_mask_fits refuses runs every row HERE: ia_gemm_wgrad_filtered hands such a shape a block mask instead)
  if (wgrad_form)
    g.live_blk = (k_mask && big && (k_steps ? t256w::step_mask_fits(g.nk_per_split) : t256w::blk_mask_fits(g.nk_per_split))) ? (const uint32_t*)c.filter.list : nullptr;
  // the list of the row-remapped forms (C2 has C's pitch, so dgrad_rows_fit covers it): a list or NULL
  const bool fwd_epi = !bks && (epilogue == EPI_BIAS || epilogue == EPI_BIAS_GELU || epilogue == EPI_BIAS_GELU_ACT || epilogue == EPI_BIAS_ADD);
  g.row_blk = nullptr; g.rows_fill = c.filter.fill ? 1 : 0; g.fill_m = M; g.rows_guarded = c.tail ? 1 : 0;
  if (row_list && !aks && !f32 && (epilogue == EPI_NONE || epilogue == EPI_ADD || epilogue == EPI_DGELU_CS || fwd_epi) && big && !g.dbg && !(N & 7) &&
      dgrad_rows_fit(M, c.lda, c.ldc, c.aux ? c.ldaux : 0))
    g.row_blk = (const int*)c.filter.list;
  // (GemmArgs::rows_grouped: 1 = a group-aligned list, 2 = a block-packed one; the column-sum epilogue only)
  g.rows_grouped = (g.row_blk && epilogue == EPI_DGELU_CS) ? (kind == IaRowFilter::GROUPS ? 1 : kind == IaRowFilter::PACKED ? 2 : 0) : 0;
  // Scaled columns, M no multiple of 128: the dense kernel rounds the rows behind the last whole 128-row part of M as (acc + bias) * scale
  // (guarded row-layout epilogue) and the others as acc * scale + bias * scale (accumulator-layout epilogue).  The remap would mix the two
  // in one wave, so the remapped launch covers the whole parts and the (at most four) blocks behind them get a remapped launch of their
  // own in front of it: one M-tile taken from the end of the live list, the row-layout epilogue in every wave (GemmCall::tail: that call,
  // GemmArgs::rows_guarded).  The fill of the main launch sees every row.
  if (g.row_blk && fwd_epi && c.qcols > 0 && (M & 127) && !c.tail) {
    GemmCall t{c.A, 0, c.lda, c.B, 0, c.ldb, c.C, 0, c.ldc, M, N, K};
    t.epilogue = epilogue; t.bias = c.bias; t.qcols = c.qcols; t.qscale = c.qscale; t.filter = c.filter; t.filter.fill = false; t.tail = true;
    int rc = gemm_core(t, stream);
    if (rc) return rc;
    const int Mb = M & ~127;
    g.a_bytes = ((uint64_t)(Mb - 1) * c.lda + K) * 2;
    g.M = Mb;
  }
  const bool needs_bias = epilogue == EPI_BIAS || epilogue == EPI_BIAS_GELU || epilogue == EPI_BIAS_GELU_ACT || epilogue == EPI_BIAS_ADD;
  const bool needs_aux = epilogue == EPI_ADD || epilogue == EPI_DGELU || epilogue == EPI_BIAS_ADD || epilogue == EPI_DGELU_CS;
  if (needs_bias && !c.bias) return IA_ERR_ARG;
  if (needs_aux && (!c.aux || (c.ldaux & 3))) return IA_ERR_ARG;
  if (epilogue == EPI_BIAS_GELU && !c.C2) return IA_ERR_ARG;

  if (!aks && !bks && !f32) {
    switch (epilogue) {
      case EPI_NONE: return launch<false, false, EPI_NONE, false>(g, big, stream, kind);
      case EPI_BIAS: return launch<false, false, EPI_BIAS, false>(g, big, stream, kind);
      case EPI_BIAS_GELU: return launch<false, false, EPI_BIAS_GELU, false>(g, big, stream, kind);
      case EPI_BIAS_GELU_ACT: return launch<false, false, EPI_BIAS_GELU_ACT, false>(g, big, stream, kind);
      case EPI_BIAS_ADD: return launch<false, false, EPI_BIAS_ADD, false>(g, big, stream, kind);
      case EPI_ADD: return launch<false, false, EPI_ADD, false>(g, big, stream, kind);
      // (the data-gradient epilogues on a k-contiguous B: the transposed weight shadows of ia_layer_weights::wt_*)
      case EPI_DGELU: return launch<false, false, EPI_DGELU, false>(g, big, stream);
      case EPI_DGELU_CS: return launch_dgelu_colsum<false>(g, big, (float*)c.C2, c.workspace, c.workspace_bytes, stream);
    }
  } else if (!aks && bks && !f32) {
    switch (epilogue) {
      case EPI_NONE: return launch<false, true, EPI_NONE, false>(g, big, stream, kind);
      case EPI_ADD: return launch<false, true, EPI_ADD, false>(g, big, stream, kind);
      case EPI_DGELU: return launch<false, true, EPI_DGELU, false>(g, big, stream);
      case EPI_DGELU_CS: return launch_dgelu_colsum<true>(g, big, (float*)c.C2, c.workspace, c.workspace_bytes, stream);
    }
  } else if (aks && bks && f32) {
    if (epilogue == EPI_NONE) {
      int rc = launch<true, true, EPI_NONE, true>(g, big, stream, kind);
      // 256x256 kernel: no spare accumulators for the row sums -> the stand-alone column-sum pass over A (stream-ordered after the
      // split-K reduce, so it may reuse the workspace)
      if (!rc && c.C2 && big) rc = ia_colsum(c.A, c.lda, K, M, (float*)c.C2, 1, c.workspace, c.workspace_bytes, stream);
      return rc;
    }
  } else if (!aks && !bks && f32) {
    if (epilogue == EPI_NONE) return launch<false, false, EPI_NONE, true>(g, big, stream);
    if (epilogue == EPI_BIAS) return launch<false, false, EPI_BIAS, true>(g, big, stream);
  }
  return IA_ERR_UNSUPPORTED;
}


// Start recording HIP events around every launch of GEMM instantiation `variant` (at most max_launches).
extern "C" int ia_prof_begin(int variant, int max_launches) {
  (void)hipGetLastError();
  if (max_launches <= 0) return IA_ERR_ARG;
  if (g_prof.cap < max_launches) {
    for (int i = 0; i < 2 * g_prof.cap; ++i) (void)hipEventDestroy(g_prof.ev[i]);
    delete[] g_prof.ev;
    g_prof.ev = new hipEvent_t[2 * max_launches];
    for (int i = 0; i < 2 * max_launches; ++i)
      if (hipEventCreate(&g_prof.ev[i]) != hipSuccess) return IA_ERR_LAUNCH;
    g_prof.cap = max_launches;
  }
  g_prof.variant = variant; g_prof.n = 0; g_prof.flops = 0.0; g_prof.bytes = 0.0; g_prof.on = true;
  return IA_OK;
}

// Stop recording; synchronises on the recorded events and returns summed kernel time, FLOPs and launch count.
extern "C" int ia_prof_end(double* total_ms, double* total_flops, int* launches) {
  (void)hipGetLastError();
  g_prof.on = false;
  double ms = 0.0;
  for (int i = 0; i < g_prof.n; ++i) {
    if (hipEventSynchronize(g_prof.ev[2 * i + 1]) != hipSuccess) return IA_ERR_LAUNCH;
    float t = 0.f;
    if (hipEventElapsedTime(&t, g_prof.ev[2 * i], g_prof.ev[2 * i + 1]) != hipSuccess) return IA_ERR_LAUNCH;
    ms += t;
  }
  if (total_ms) *total_ms = ms;
  if (total_flops) *total_flops = g_prof.flops;
  if (launches) *launches = g_prof.n;
  return IA_OK;
}

// Diagnostics: `workgroups` workgroups that each take a whole CU's LDS and spin for `milliseconds` (100 MHz wall clock)
namespace {
__global__ __launch_bounds__(256) void cu_hog_kernel(unsigned long long ticks) {
  extern __shared__ __attribute__((aligned(16))) char hog_smem[];
  if (threadIdx.x == 0) *reinterpret_cast<volatile int*>(hog_smem) = 1;      // the allocation is real
  const unsigned long long t0 = wall_clock64();
  while (wall_clock64() - t0 < ticks) __builtin_amdgcn_s_sleep(32);
}
}  // namespace
// Diagnostics: switch the dynamic tile claim of the persistent GEMM launches on / off at run time (the IA_GEMM_DYNAMIC default otherwise);
// returns the previous setting.
extern "C" int ia_debug_gemm_dynamic(int on) {
  if (g_dynamic < 0) (void)next_ctr_slot();
  const int prev = g_dynamic;
  if (on >= 0) g_dynamic = on ? 1 : 0;        // (negative: query only)
  return prev;
}
extern "C" int ia_debug_cu_hog(int workgroups, float milliseconds, hipStream_t stream) {
  (void)hipGetLastError();
  if (workgroups <= 0 || workgroups > 256 || !(milliseconds > 0.f) || milliseconds > 1000.f) return IA_ERR_ARG;
  static bool attr_set = false;
  if (!attr_set) {
    if (hipFuncSetAttribute((const void*)cu_hog_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, t256w::LDS_BYTES) != hipSuccess) return IA_ERR_LAUNCH;
    attr_set = true;
  }
  hipLaunchKernelGGL(cu_hog_kernel, dim3(workgroups), dim3(256), t256w::LDS_BYTES, stream, (unsigned long long)(milliseconds * 1e5f));
  return ia_check_launch();
}

// algorithmic bytes (each operand read once, the output written once) of the launches recorded between ia_prof_begin / ia_prof_end
extern "C" double ia_prof_bytes(void) { return g_prof.bytes; }
