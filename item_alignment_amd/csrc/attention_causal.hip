// Causal multi-query attention for the CoCa decoder blocks (ParallelTransformerBlock(is_decoding=True), reference
// src/models/multimodal.py:529-626 with the triu mask of :575-583), head dim 64, gfx950.
//
//   O = softmax(Q K^T * scale + causal) V,   query row i of a sequence (0 <= i < Lq = fold * Lk) attends key j  iff  j <= i / fold.
// fold = 1 is ordinary causal self-attention; the decoder block folds its query heads into rows (row r = token r / heads), so it is the
// fold = heads, nh = 1 case.  No key mask, no dropout (the reference block has neither).
//
// The mask belongs to a (query, key) pair, so it cannot ride on the per-tile key ballot of attention.hip: it is applied element by
// element, but only in the 32-key blocks that cross the diagonal of a wave's 32 queries; blocks wholly above it are not multiplied,
// 64-key tiles wholly above a workgroup's diagonal are not fetched.
//
// Numerics are those of attention.hip (so the bars of tests/attn_reference.py carry over): K meets q' = bf16(q * scale * log2 e), the
// softmax runs in the exp2 domain in fp32, P is packed to bf16 for the PV / dV / dS products and the row sum is taken from the packed
// values, outputs are bf16; the backward recomputes P = exp2(s - lse2) and takes delta = rowsum(dO o O) from the stored context.
// One difference, which stays inside those bars: the softmax reference is the running maximum rounded up to an integer (subtracted in
// fp32 on the VALU; moving it rescales the accumulators by an exact power of two), not the lazy bf16 reference of attn_fwd3_kernel.
//
// Orientation as in attention.hip: the forward and the dQ side are computed transposed, S^T[key][q] = K Q'^T (MFMA 32x32x16, A = K
// rows from LDS, B = Q' rows in registers), so a lane owns one query (q = lane & 31) and softmax statistics are lane-local up to the
// partner lane ^ 32; P^T / dS^T go from the accumulators straight into the B operand of the next product.  The A operand of that
// product is a TRANSPOSED tile (V^T, K^T, dO^T, Q'^T): the staging code writes it transposed into LDS (plain 2-byte stores), and a lane
// reads its eight k-slots as two 8-byte pieces in the order the accumulator layout dictates (k-slot (half, j) <-> row
// (j & 3) + 8 (j >> 2) + 4 half of the 16-row step).  Everything here is plain HIP C++ plus the MFMA builtin: no LDS-DMA, no inline
// asm, no counted waits (nothing for tools/lint_asm_waits.py to check).
//
// Three kernels:
//   attn_causal_fwd_kernel   workgroup = 128 queries (4 waves x 32), streams the key tiles 0 .. diagonal
//   attn_causal_dq_kernel    the same walk; dQ^T += K^T dS^T; leaves delta behind
//   attn_causal_dkv_kernel   workgroup = 32 keys; its 4 waves take the 32-query blocks from the diagonal down in turn (block qb0 + 4 it +
//                            wave), then the four partial dK^T / dV^T are added in wave order through LDS: a fixed order, no atomics
#include "common.h"

namespace {

constexpr float LOG2E = 1.4426950408889634f;
constexpr float NEG_BIG = -1e30f;
constexpr int MAX_LK = 2048;
constexpr int LDT = 72;      // padded row (elements) of a staged 64 x 64 tile: 144 B keeps 16-byte reads aligned and rows off each other's banks
constexpr int LDW = 40;      // padded row (elements) of a wave's transposed 64 x 32 tile (dK/dV kernel): 80 B, 8-byte aligned

// row index inside a 32-row accumulator block for register r of lane-half hh
#define CA_ROW(r, hh) (((r) & 3) + 8 * ((r) >> 2) + 4 * (hh))

struct CausalArgs {
  const bf16* q; const bf16* k; const bf16* v;   // q rows b*Lq + i, k / v rows b*Lk + j, head h at column h*64
  const bf16* o; const bf16* d_o;
  bf16* out; bf16* dq; bf16* dk; bf16* dv;
  float* lse2; float* delta;                      // [B, nh, Lq]
  int B, nh, Lq, Lk, fold;
  int ld_q, ld_kv, ld_o, ld_dq, ld_dkv;
  float sc, scale;                                // scale * log2(e), scale
};

IA_DEV f32x16 mfma(bf16x8 a, bf16x8 b, f32x16 c) { return __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, c, 0, 0, 0); }
IA_DEV f32x16 zero16() {
  f32x16 z;
#pragma unroll
  for (int i = 0; i < 16; ++i) z[i] = 0.f;
  return z;
}
IA_DEV bf16x8 zero8() {
  bf16x8 z;
#pragma unroll
  for (int i = 0; i < 8; ++i) z[i] = f2bf(0.f);
  return z;
}
// eight bf16 of row `row` from column `col` on; zeros when the row does not exist
IA_DEV bf16x8 load8(const bf16* base, size_t row, int ld, int col, bool ok) {
  return ok ? *reinterpret_cast<const bf16x8*>(base + row * (size_t)ld + col) : zero8();
}
IA_DEV bf16x8 prescale(bf16x8 raw, float sc) {
  bf16x8 r;
#pragma unroll
  for (int j = 0; j < 8; ++j) r[j] = f2bf(bf2f(raw[j]) * sc);
  return r;
}
IA_DEV float xor32(float x) { return __shfl_xor(x, 32, 64); }
// A^T fragment of one 16-row step out of a transposed tile t[col][row] (row stride ld elements): column `col`, rows row0 + {0..3, 8..11}
// + 4 half
IA_DEV bf16x8 frag_t(const bf16* t, int ld, int col, int row0, int half) {
  const bf16x4 lo = *reinterpret_cast<const bf16x4*>(t + col * ld + row0 + 4 * half);
  const bf16x4 hi = *reinterpret_cast<const bf16x4*>(t + col * ld + row0 + 4 * half + 8);
  return bf16x8{lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
}
// a lane's 16 + 16 values of one output row (accumulator blocks a0: columns 0..31, a1: 32..63 of row `dst`), times mul, as bf16
IA_DEV void store_row(bf16* dst, const f32x16& a0, const f32x16& a1, float mul, int hh) {
#pragma unroll
  for (int g = 0; g < 4; ++g) {
    bf16x4 x, y;
#pragma unroll
    for (int j = 0; j < 4; ++j) { x[j] = f2bf(a0[g * 4 + j] * mul); y[j] = f2bf(a1[g * 4 + j] * mul); }
    *reinterpret_cast<bf16x4*>(dst + 8 * g + 4 * hh) = x;
    *reinterpret_cast<bf16x4*>(dst + 32 + 8 * g + 4 * hh) = y;
  }
}
IA_DEV void block_coords(int nt, int nh, int& tile, int& h, int& b) {
  int w = blockIdx.x;
  tile = w % nt; w /= nt;
  h = w % nh; b = w / nh;
}

// One 64-key tile in flight: 256 threads x 2 pieces of 16 bytes per operand.  K pieces are dealt row-major (8 lanes = one 128-byte
// row); pieces that are written TRANSPOSED are dealt key-major (64 lanes = 64 keys of one 8-column chunk), so the 2-byte LDS
// stores of a wave fall on consecutive addresses.
struct TileRegs { bf16x8 a[2], b[2]; };
IA_DEV void piece_rm(int tid, int i, int& row, int& ch) { const int c = tid + i * 256; row = c >> 3; ch = c & 7; }
IA_DEV void piece_km(int tid, int i, int& row, int& ch) { const int c = tid + i * 256; row = c & 63; ch = c >> 6; }
IA_DEV void put_rows(bf16* t, int row, int ch, bf16x8 x) { *reinterpret_cast<bf16x8*>(t + row * LDT + ch * 8) = x; }
IA_DEV void put_transposed(bf16* t, int row, int ch, bf16x8 x) {
#pragma unroll
  for (int j = 0; j < 8; ++j) t[(ch * 8 + j) * LDT + row] = x[j];
}

// ------------------------------------------------------------------------------------------ forward
__global__ __launch_bounds__(256) void attn_causal_fwd_kernel(CausalArgs p) {
  __shared__ __attribute__((aligned(16))) bf16 sK[64 * LDT];     // [key][d]
  __shared__ __attribute__((aligned(16))) bf16 sVt[64 * LDT];    // [d][key]
  const int tid = threadIdx.x, lane = tid & 63, hh = lane >> 5, lq = lane & 31, wave = tid >> 6;
  int tile, h, b;
  block_coords((p.Lq + 127) >> 7, p.nh, tile, h, b);
  const int Lq = p.Lq, Lk = p.Lk, fold = p.fold;
  const size_t qbase = (size_t)b * Lq, kbase = (size_t)b * Lk;
  const int Q0 = tile * 128, q0 = Q0 + wave * 32, qi = q0 + lq;
  const bool active = q0 < Lq;                                   // wave-uniform
  const int tok = qi / fold;                                     // the last key this lane's query attends
  const int tok_lo = q0 / fold, tok_hi = (q0 + 31 < Lq ? q0 + 31 : Lq - 1) / fold;      // of the wave's first / last existing query
  const int ntile = ((Q0 + 127 < Lq ? Q0 + 127 : Lq - 1) / fold) / 64 + 1;               // key tiles up to the workgroup's diagonal
  const int col = h * 64;

  bf16x8 qf[4];
#pragma unroll
  for (int kb = 0; kb < 4; ++kb) qf[kb] = prescale(load8(p.q, qbase + qi, p.ld_q, col + kb * 16 + hh * 8, qi < Lq), p.sc);

  TileRegs tr;
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    int row, ch;
    piece_rm(tid, i, row, ch); tr.a[i] = load8(p.k, kbase + row, p.ld_kv, col + ch * 8, row < Lk);
    piece_km(tid, i, row, ch); tr.b[i] = load8(p.v, kbase + row, p.ld_kv, col + ch * 8, row < Lk);
  }
  f32x16 o0 = zero16(), o1 = zero16();
  float m_run = NEG_BIG, l_run = 0.f;                            // l_run: this lane's half of the row sum (in units of 2^m_run)

  for (int t = 0; t < ntile; ++t) {
    __syncthreads();                                             // everybody has finished reading tile t-1
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      int row, ch;
      piece_rm(tid, i, row, ch); put_rows(sK, row, ch, tr.a[i]);
      piece_km(tid, i, row, ch); put_transposed(sVt, row, ch, tr.b[i]);
    }
    __syncthreads();
    if (t + 1 < ntile) {                                         // the next tile travels under this tile's arithmetic
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        int row, ch;
        piece_rm(tid, i, row, ch); row += (t + 1) * 64; tr.a[i] = load8(p.k, kbase + row, p.ld_kv, col + ch * 8, row < Lk);
        piece_km(tid, i, row, ch); row += (t + 1) * 64; tr.b[i] = load8(p.v, kbase + row, p.ld_kv, col + ch * 8, row < Lk);
      }
    }
    if (!active) continue;
#pragma unroll
    for (int blk = 0; blk < 2; ++blk) {
      const int j0 = t * 64 + blk * 32;
      if (j0 > tok_hi) break;                                    // wholly above this wave's diagonal (wave-uniform)
      f32x16 s = zero16();
#pragma unroll
      for (int kb = 0; kb < 4; ++kb)
        s = mfma(*reinterpret_cast<const bf16x8*>(sK + (blk * 32 + lq) * LDT + kb * 16 + hh * 8), qf[kb], s);
      if (j0 + 31 > tok_lo) {                                    // the block crosses the diagonal: per-element mask
#pragma unroll
        for (int r = 0; r < 16; ++r)
          if (j0 + CA_ROW(r, hh) > tok) s[r] = NEG_BIG;
      }
      float tm = s[0];
#pragma unroll
      for (int r = 1; r < 16; ++r) tm = fmaxf(tm, s[r]);
      tm = fmaxf(tm, xor32(tm));
      // The softmax reference is an INTEGER (log2 units) no smaller than the running maximum, finite from block 0 on (key 0 is
      // attendable for every query): moving it multiplies what has been accumulated by a power of two, which is exact -- the online
      // softmax adds no rounding site to those of attn_fwd3_kernel.  (-200: the first block, where there is nothing accumulated yet,
      // and any move so large that the old sums vanish in fp32 either way.)
      const float m_new = fmaxf(m_run, ceilf(tm));
      const int shift = (int)fmaxf(m_run - m_new, -200.f);
      bf16x8 pa, pb;
      float rs = 0.f;
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        pa[j] = f2bf(__builtin_amdgcn_exp2f(s[j] - m_new));
        pb[j] = f2bf(__builtin_amdgcn_exp2f(s[8 + j] - m_new));
        rs += bf2f(pa[j]) + bf2f(pb[j]);                         // the row sum of the ROUNDED values: O is a convex combination of v rows
      }
      l_run = __builtin_ldexpf(l_run, shift) + rs;
      m_run = m_new;
      if (shift != 0) {
#pragma unroll
        for (int r = 0; r < 16; ++r) { o0[r] = __builtin_ldexpf(o0[r], shift); o1[r] = __builtin_ldexpf(o1[r], shift); }
      }
      o0 = mfma(frag_t(sVt, LDT, lq, blk * 32, hh), pa, o0);
      o1 = mfma(frag_t(sVt, LDT, 32 + lq, blk * 32, hh), pa, o1);
      o0 = mfma(frag_t(sVt, LDT, lq, blk * 32 + 16, hh), pb, o0);
      o1 = mfma(frag_t(sVt, LDT, 32 + lq, blk * 32 + 16, hh), pb, o1);
    }
  }
  if (!active || qi >= Lq) return;
  const float l_tot = l_run + xor32(l_run);
  if (hh == 0) p.lse2[((size_t)b * p.nh + h) * Lq + qi] = m_run + __builtin_amdgcn_logf(l_tot);      // v_log_f32 = log2
  store_row(p.out + (qbase + qi) * (size_t)p.ld_o + col, o0, o1, 1.0f / l_tot, hh);
}

// ------------------------------------------------------------------------------------- backward: dQ
__global__ __launch_bounds__(256) void attn_causal_dq_kernel(CausalArgs p) {
  __shared__ __attribute__((aligned(16))) bf16 sK[64 * LDT];     // [key][d]
  __shared__ __attribute__((aligned(16))) bf16 sV[64 * LDT];     // [key][d]
  __shared__ __attribute__((aligned(16))) bf16 sKt[64 * LDT];    // [d][key]
  const int tid = threadIdx.x, lane = tid & 63, hh = lane >> 5, lq = lane & 31, wave = tid >> 6;
  int tile, h, b;
  block_coords((p.Lq + 127) >> 7, p.nh, tile, h, b);
  const int Lq = p.Lq, Lk = p.Lk, fold = p.fold;
  const size_t qbase = (size_t)b * Lq, kbase = (size_t)b * Lk;
  const int Q0 = tile * 128, q0 = Q0 + wave * 32, qi = q0 + lq;
  const bool active = q0 < Lq, have = qi < Lq;
  const int tok = qi / fold;
  const int tok_lo = q0 / fold, tok_hi = (q0 + 31 < Lq ? q0 + 31 : Lq - 1) / fold;
  const int ntile = ((Q0 + 127 < Lq ? Q0 + 127 : Lq - 1) / fold) / 64 + 1;
  const int col = h * 64;
  const size_t sidx = ((size_t)b * p.nh + h) * Lq + (have ? qi : 0);

  bf16x8 qf[4], gf[4];
  float dl = 0.f;
#pragma unroll
  for (int kb = 0; kb < 4; ++kb) {
    const int c = col + kb * 16 + hh * 8;
    qf[kb] = prescale(load8(p.q, qbase + qi, p.ld_q, c, have), p.sc);
    gf[kb] = load8(p.d_o, qbase + qi, p.ld_o, c, have);
    const bf16x8 of = load8(p.o, qbase + qi, p.ld_o, c, have);
#pragma unroll
    for (int j = 0; j < 8; ++j) dl += bf2f(gf[kb][j]) * bf2f(of[j]);
  }
  const float delta = dl + xor32(dl);                            // rowsum(dO o O) from the stored context
  const float lse = have ? p.lse2[sidx] : 0.f;
  if (have && hh == 0) p.delta[sidx] = delta;

  TileRegs tk, tv;                                               // tk.a: K row-major pieces, tk.b: K key-major pieces (transposed store), tv.a: V
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    int row, ch;
    piece_rm(tid, i, row, ch);
    tk.a[i] = load8(p.k, kbase + row, p.ld_kv, col + ch * 8, row < Lk);
    tv.a[i] = load8(p.v, kbase + row, p.ld_kv, col + ch * 8, row < Lk);
    piece_km(tid, i, row, ch);
    tk.b[i] = load8(p.k, kbase + row, p.ld_kv, col + ch * 8, row < Lk);
  }
  f32x16 d0 = zero16(), d1 = zero16();

  for (int t = 0; t < ntile; ++t) {
    __syncthreads();
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      int row, ch;
      piece_rm(tid, i, row, ch); put_rows(sK, row, ch, tk.a[i]); put_rows(sV, row, ch, tv.a[i]);
      piece_km(tid, i, row, ch); put_transposed(sKt, row, ch, tk.b[i]);
    }
    __syncthreads();
    if (t + 1 < ntile) {
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        int row, ch;
        piece_rm(tid, i, row, ch); row += (t + 1) * 64;
        tk.a[i] = load8(p.k, kbase + row, p.ld_kv, col + ch * 8, row < Lk);
        tv.a[i] = load8(p.v, kbase + row, p.ld_kv, col + ch * 8, row < Lk);
        piece_km(tid, i, row, ch); row += (t + 1) * 64;
        tk.b[i] = load8(p.k, kbase + row, p.ld_kv, col + ch * 8, row < Lk);
      }
    }
    if (!active) continue;
#pragma unroll
    for (int blk = 0; blk < 2; ++blk) {
      const int j0 = t * 64 + blk * 32;
      if (j0 > tok_hi) break;
      f32x16 s = zero16(), dp = zero16();
#pragma unroll
      for (int kb = 0; kb < 4; ++kb) {
        s = mfma(*reinterpret_cast<const bf16x8*>(sK + (blk * 32 + lq) * LDT + kb * 16 + hh * 8), qf[kb], s);
        dp = mfma(*reinterpret_cast<const bf16x8*>(sV + (blk * 32 + lq) * LDT + kb * 16 + hh * 8), gf[kb], dp);
      }
      const bool crossing = j0 + 31 > tok_lo;
      bf16x8 da, db;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        float pr = __builtin_amdgcn_exp2f(s[r] - lse);
        if (crossing && j0 + CA_ROW(r, hh) > tok) pr = 0.f;      // select, not multiply: a masked score may be anything
        const bf16 ds = f2bf(pr * (dp[r] - delta));
        if (r < 8) da[r] = ds; else db[r - 8] = ds;
      }
      d0 = mfma(frag_t(sKt, LDT, lq, blk * 32, hh), da, d0);
      d1 = mfma(frag_t(sKt, LDT, 32 + lq, blk * 32, hh), da, d1);
      d0 = mfma(frag_t(sKt, LDT, lq, blk * 32 + 16, hh), db, d0);
      d1 = mfma(frag_t(sKt, LDT, 32 + lq, blk * 32 + 16, hh), db, d1);
    }
  }
  if (!active || !have) return;
  store_row(p.dq + (qbase + qi) * (size_t)p.ld_dq + col, d0, d1, p.scale, hh);
}

// -------------------------------------------------------------------------------- backward: dK, dV
// S orientation: S[q][key] = Q' K^T (A = Q' rows, B = K rows, both straight from global memory into registers), so a lane owns one key
// (lane & 31) and its 16 registers are 16 queries of the block; lse2 / delta of those queries come from a wave-private LDS row.
constexpr int DKV_WAVE = 2 * 64 * LDW * 2 + 64 * 4;             // bytes: Q'^T | dO^T | lse2[32] delta[32]
constexpr int DKV_RED = 3 * 64 * 64 * 4;                        // bytes: the partial sums of waves 1..3 (64 registers x 64 lanes each)
constexpr int DKV_SMEM = DKV_RED > 4 * DKV_WAVE ? DKV_RED : 4 * DKV_WAVE;

__global__ __launch_bounds__(256) void attn_causal_dkv_kernel(CausalArgs p) {
  __shared__ __attribute__((aligned(16))) char smem[DKV_SMEM];
  const int tid = threadIdx.x, lane = tid & 63, hh = lane >> 5, lq = lane & 31, wave = tid >> 6;
  int tile, h, b;
  block_coords((p.Lk + 31) >> 5, p.nh, tile, h, b);
  const int Lq = p.Lq, Lk = p.Lk, fold = p.fold;
  const size_t qbase = (size_t)b * Lq, kbase = (size_t)b * Lk;
  const int j0 = tile * 32, key = j0 + lq;
  const int first_q = key * fold;                                // the first query that attends this lane's key
  const int col = h * 64;
  bf16* const sQt = reinterpret_cast<bf16*>(smem + wave * DKV_WAVE);      // [d][q]
  bf16* const sGt = sQt + 64 * LDW;                                       // [d][q]
  float* const sStat = reinterpret_cast<float*>(sGt + 64 * LDW);

  bf16x8 kf[4], vf[4];
#pragma unroll
  for (int kb = 0; kb < 4; ++kb) {
    kf[kb] = load8(p.k, kbase + key, p.ld_kv, col + kb * 16 + hh * 8, key < Lk);
    vf[kb] = load8(p.v, kbase + key, p.ld_kv, col + kb * 16 + hh * 8, key < Lk);
  }
  f32x16 dk0 = zero16(), dk1 = zero16(), dv0 = zero16(), dv1 = zero16();
  const int nqb = (Lq + 31) >> 5, qb0 = (j0 * fold) >> 5;        // query blocks qb0 .. nqb-1 hold a query that attends one of these keys
  const int niter = (nqb - qb0 + 3) >> 2;
  const size_t sbase = ((size_t)b * p.nh + h) * Lq;

  for (int it = 0; it < niter; ++it) {
    const int qb = qb0 + it * 4 + wave;
    const bool act = qb < nqb;                                   // wave-uniform
    const int qi = qb * 32 + lq;
    const bool have = act && qi < Lq;
    bf16x8 qf[4], gf[4];
#pragma unroll
    for (int kb = 0; kb < 4; ++kb) {
      qf[kb] = prescale(load8(p.q, qbase + qi, p.ld_q, col + kb * 16 + hh * 8, have), p.sc);
      gf[kb] = load8(p.d_o, qbase + qi, p.ld_o, col + kb * 16 + hh * 8, have);
    }
    const float st = have ? (hh == 0 ? p.lse2[sbase + qi] : p.delta[sbase + qi]) : 0.f;
    __syncthreads();                                             // the previous block's fragments have been read
#pragma unroll
    for (int kb = 0; kb < 4; ++kb)
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        sQt[(kb * 16 + hh * 8 + j) * LDW + lq] = qf[kb][j];
        sGt[(kb * 16 + hh * 8 + j) * LDW + lq] = gf[kb][j];
      }
    sStat[lane] = st;                                            // [0..31] lse2, [32..63] delta of the block's queries
    __syncthreads();
    if (!act) continue;
    f32x16 s = zero16(), dp = zero16();
#pragma unroll
    for (int kb = 0; kb < 4; ++kb) {
      s = mfma(qf[kb], kf[kb], s);
      dp = mfma(gf[kb], vf[kb], dp);
    }
    const bool crossing = qb * 32 < (j0 + 31) * fold;            // some (query, key) pair of the block is above the diagonal
    bf16x8 pa, pb, da, db;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int row = CA_ROW(r, hh);
      float pr = __builtin_amdgcn_exp2f(s[r] - sStat[row]);
      if (crossing && qb * 32 + row < first_q) pr = 0.f;
      const bf16 pv = f2bf(pr), ds = f2bf(pr * (dp[r] - sStat[32 + row]));
      if (r < 8) { pa[r] = pv; da[r] = ds; } else { pb[r - 8] = pv; db[r - 8] = ds; }
    }
    dv0 = mfma(frag_t(sGt, LDW, lq, 0, hh), pa, dv0);
    dv1 = mfma(frag_t(sGt, LDW, 32 + lq, 0, hh), pa, dv1);
    dv0 = mfma(frag_t(sGt, LDW, lq, 16, hh), pb, dv0);
    dv1 = mfma(frag_t(sGt, LDW, 32 + lq, 16, hh), pb, dv1);
    dk0 = mfma(frag_t(sQt, LDW, lq, 0, hh), da, dk0);
    dk1 = mfma(frag_t(sQt, LDW, 32 + lq, 0, hh), da, dk1);
    dk0 = mfma(frag_t(sQt, LDW, lq, 16, hh), db, dk0);
    dk1 = mfma(frag_t(sQt, LDW, 32 + lq, 16, hh), db, dk1);
  }
  // the four waves' partial sums, added in wave order 0 + 1 + 2 + 3 by wave 0
  __syncthreads();
  float* const red = reinterpret_cast<float*>(smem);
  if (wave > 0) {
    float* const w = red + (size_t)(wave - 1) * 64 * 64 + lane;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      w[r * 64] = dk0[r]; w[(16 + r) * 64] = dk1[r]; w[(32 + r) * 64] = dv0[r]; w[(48 + r) * 64] = dv1[r];
    }
  }
  __syncthreads();
  if (wave > 0 || key >= Lk) return;
#pragma unroll
  for (int w = 0; w < 3; ++w) {
    const float* const rd = red + (size_t)w * 64 * 64 + lane;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      dk0[r] += rd[r * 64]; dk1[r] += rd[(16 + r) * 64]; dv0[r] += rd[(32 + r) * 64]; dv1[r] += rd[(48 + r) * 64];
    }
  }
  // dK^T / dV^T: accumulator row = d, column = this lane's key; dk = sum dS q' / log2(e) with q' = bf16(q scale log2 e)
  store_row(p.dk + (kbase + key) * (size_t)p.ld_dkv + col, dk0, dk1, 1.0f / LOG2E, hh);
  store_row(p.dv + (kbase + key) * (size_t)p.ld_dkv + col, dv0, dv1, 1.0f, hh);
}

bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// argument checks shared by the two entry points; Lq = fold * Lk
int fill(CausalArgs& a, int B, int nh, int Lk, int fold, int ld_q, int ld_kv, int ld_o, float scale) {
  if (B <= 0 || nh <= 0 || Lk <= 0 || fold <= 0 || Lk > MAX_LK) return IA_ERR_ARG;
  if ((long)fold * Lk > (1 << 20) || (long)B * nh > (1 << 20)) return IA_ERR_ARG;
  if ((ld_q & 7) || (ld_kv & 7) || (ld_o & 7) || ld_q < nh * 64 || ld_kv < nh * 64 || ld_o < nh * 64) return IA_ERR_ARG;
  a.B = B; a.nh = nh; a.Lk = Lk; a.fold = fold; a.Lq = fold * Lk;
  a.ld_q = ld_q; a.ld_kv = ld_kv; a.ld_o = ld_o; a.ld_dq = ld_q; a.ld_dkv = ld_kv;
  a.scale = scale; a.sc = scale * LOG2E;
  return IA_OK;
}

}  // namespace

// Causal form of ia_attn_fwd_x: Lq = fold * Lk queries, query i attends key j iff j <= i / fold; no key mask, no dropout.
extern "C" int ia_attn_fwd_causal_x(const void* q, int ld_q, const void* k, const void* v, int ld_kv, void* out, int ld_o, float* lse2, int B,
                                    int nh, int Lk, int fold, float scale, hipStream_t stream) {
  (void)hipGetLastError();  // drop stale status left by unrelated runtime calls
  if (!q || !k || !v || !out || !lse2) return IA_ERR_ARG;
  if (!aligned16(q) || !aligned16(k) || !aligned16(v) || !aligned16(out)) return IA_ERR_ARG;
  CausalArgs a{};
  const int rc = fill(a, B, nh, Lk, fold, ld_q, ld_kv, ld_o, scale);
  if (rc) return rc;
  a.q = (const bf16*)q; a.k = (const bf16*)k; a.v = (const bf16*)v; a.out = (bf16*)out; a.lse2 = lse2;
  hipLaunchKernelGGL(attn_causal_fwd_kernel, dim3(((a.Lq + 127) / 128) * nh * B), dim3(256), 0, stream, a);
  return ia_check_launch();
}

// delta: caller-provided scratch of B*nh*Lq floats (filled by the dQ kernel, read by the dK/dV kernel).
extern "C" int ia_attn_bwd_causal_x(const void* q, int ld_q, const void* k, const void* v, int ld_kv, const void* out, const void* d_out,
                                    int ld_o, const float* lse2, float* delta, void* dq, int ld_dq, void* dk, void* dv, int ld_dkv, int B,
                                    int nh, int Lk, int fold, float scale, hipStream_t stream) {
  (void)hipGetLastError();
  if (!q || !k || !v || !out || !d_out || !lse2 || !delta || !dq || !dk || !dv) return IA_ERR_ARG;
  if (!aligned16(q) || !aligned16(k) || !aligned16(v) || !aligned16(out) || !aligned16(d_out) || !aligned16(dq) || !aligned16(dk) ||
      !aligned16(dv))
    return IA_ERR_ARG;
  CausalArgs a{};
  const int rc = fill(a, B, nh, Lk, fold, ld_q, ld_kv, ld_o, scale);
  if (rc) return rc;
  if ((ld_dq & 7) || (ld_dkv & 7) || ld_dq < nh * 64 || ld_dkv < nh * 64) return IA_ERR_ARG;
  a.q = (const bf16*)q; a.k = (const bf16*)k; a.v = (const bf16*)v; a.o = (const bf16*)out; a.d_o = (const bf16*)d_out;
  a.lse2 = const_cast<float*>(lse2); a.delta = delta;
  a.dq = (bf16*)dq; a.dk = (bf16*)dk; a.dv = (bf16*)dv; a.ld_dq = ld_dq; a.ld_dkv = ld_dkv;
  hipLaunchKernelGGL(attn_causal_dq_kernel, dim3(((a.Lq + 127) / 128) * nh * B), dim3(256), 0, stream, a);
  hipLaunchKernelGGL(attn_causal_dkv_kernel, dim3(((Lk + 31) / 32) * nh * B), dim3(256), 0, stream, a);
  return ia_check_launch();
}
