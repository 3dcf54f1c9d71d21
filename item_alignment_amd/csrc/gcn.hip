// GCNII graph encoder of the graph two-tower model (reference src/models/graph.py: GCN over the item / attribute-value graph,
// torch_geometric GCN2Conv with shared_weights=True, normalize=False), full-graph forward and backward, fp32 throughout.
//
//   input layer   x_0 = relu(drop(X) W_in^T + b)                                 ia_gcn_input_fwd / _bwd
//   layer l       h   = (1 - alpha) A drop(x) + alpha x_0                        ia_gcn_propagate_fwd / _bwd
//                 x   = [drop] relu((1 - beta_l) h + beta_l h W_l)               ia_gcn_mix_fwd / _bwd
//   pair stage    rows of the node embeddings picked by index, head dropout      ia_gcn_pair_gather_fwd / ia_gcn_pair_scatter_bwd
//
// Every dropout mask is a function of (seed, stream, element index) through ia_rng (two 16-bit draws per hash, element e takes the
// low half for even e), so the backward regenerates it and nothing but x_0, h and the layer outputs is kept.  A layer output that
// was dropped (the last one) is > 0 exactly where relu' = 1 AND the element was kept, so the output itself is the only "sign"
// the backward needs.
//
// No float atomics: a CSR row is summed neighbour by neighbour in index order by one wave (even / odd neighbours on the two
// half-waves when a row of x fits 32 lanes of float4), rows longer than GCN_LONG are cut into 16 contiguous chunks summed by the
// 16 waves of a workgroup and joined through LDS in chunk order; the weight gradients are per-slab partial products joined in slab
// order.  The results are bit-identical from run to run.  The backward of the propagation is the same gather on the CSR of A^T.
#include "common.h"
#include "../../include/itemalign.h"

namespace {

constexpr int GCN_LONG = 512;    // rows with more neighbours than this are split across the waves of a workgroup
constexpr int GCN_WAVES = 16;    // waves per workgroup of the propagate kernel = short rows per workgroup = chunks of a long row
constexpr int GCN_SLAB = 1024;   // node rows per partial slab of the weight-gradient products (IA_GCN_SLAB_ROWS)
constexpr int GCN_MAXC = 512;

struct GcnDrop { uint32_t thr16; float inv_keep; uint32_t seed, stream; };

GcnDrop gcn_drop(float p, uint32_t seed, uint32_t stream) {
  GcnDrop d;
  d.thr16 = p > 0.f ? (uint32_t)(p * 65536.f + 0.5f) : 0u;
  d.inv_keep = p > 0.f ? 1.f / (1.f - (float)d.thr16 / 65536.f) : 1.f;
  d.seed = seed; d.stream = stream;
  return d;
}

// keep flags of elements e .. e+3 (e % 4 == 0) as multipliers `on` / 0
IA_DEV f32x4 gcn_keep4(const GcnDrop& d, uint32_t e, float on) {
  if (!d.thr16) return f32x4{on, on, on, on};
  const uint32_t r0 = ia_rng(d.seed, d.stream, e >> 1), r1 = ia_rng(d.seed, d.stream, (e >> 1) + 1);
  f32x4 k;
  k[0] = (r0 & 0xFFFFu) >= d.thr16 ? on : 0.f;
  k[1] = (r0 >> 16) >= d.thr16 ? on : 0.f;
  k[2] = (r1 & 0xFFFFu) >= d.thr16 ? on : 0.f;
  k[3] = (r1 >> 16) >= d.thr16 ? on : 0.f;
  return k;
}
IA_DEV f32x4 ld4(const float* p) { return *reinterpret_cast<const f32x4*>(p); }
IA_DEV void st4(float* p, const f32x4& v) { *reinterpret_cast<f32x4*>(p) = v; }
IA_DEV f32x4 zero4() { return f32x4{0.f, 0.f, 0.f, 0.f}; }

// ------------------------------------------------------------------------------------------------ propagation
// HALF (C <= 128): lane & 31 owns columns 4 (lane & 31) .. +3, the two half-waves take alternate neighbours, 4 each per step
// (8 rows of x in flight per wave).  Otherwise lane owns columns 4 lane + 256 k, k < 2, and the wave takes 4 neighbours per step.
// acc = sum over neighbours q in [lo, hi) of val[q] * keep(col[q], c) * x[col[q]][c]     (keep = 1 in the backward form)
template <bool HALF, bool COL64, bool BWD>
IA_DEV void gcn_row_sum(const void* __restrict__ col, const float* __restrict__ val, const float* __restrict__ x, long lo, long hi, int N, int C,
                        const GcnDrop& d, int lane, f32x4 (&acc)[2]) {
  constexpr int NV = HALF ? 1 : 2;
  constexpr int STEP = HALF ? 2 : 1;
  const int sub = HALF ? (lane >> 5) : 0;
  const int c0 = HALF ? (lane & 31) * 4 : lane * 4;
  acc[0] = zero4(); acc[1] = zero4();
  for (long q = lo + sub; q < hi; q += 4 * STEP) {
    f32x4 v[4][NV];
    float a[4];
    long j[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const long qq = q + u * STEP;
      const bool in = qq < hi;
      long jj = 0;
      if (in) jj = COL64 ? (long)reinterpret_cast<const int64_t*>(col)[qq] : (long)reinterpret_cast<const int32_t*>(col)[qq];
      const bool ok = in && jj >= 0 && jj < N;          // an index outside the graph contributes nothing (and reads nothing)
      a[u] = ok ? (val ? val[qq] : 1.f) : 0.f;
      j[u] = ok ? jj : 0;
#pragma unroll
      for (int k = 0; k < NV; ++k) {
        const int c = c0 + 256 * k;
        v[u][k] = c < C ? ld4(x + (size_t)j[u] * C + c) : zero4();
      }
    }
#pragma unroll
    for (int u = 0; u < 4; ++u)
#pragma unroll
      for (int k = 0; k < NV; ++k) {
        const int c = c0 + 256 * k;
        f32x4 w = v[u][k];
        if (!BWD && d.thr16 && c < C) w = w * gcn_keep4(d, (uint32_t)j[u] * (uint32_t)C + (uint32_t)c, 1.f);
#pragma unroll
        for (int e = 0; e < 4; ++e) acc[k][e] = fmaf(a[u], w[e], acc[k][e]);
      }
  }
  if (HALF) {
#pragma unroll
    for (int e = 0; e < 4; ++e) acc[0][e] = ia_add_xor32(acc[0][e]);     // even-neighbour + odd-neighbour sums, the same in both halves
  }
}

// forward:  h[row] = c_prop * acc + alpha * x0[row],  c_prop = (1 - alpha) / keep
// backward: dx[row] = keep(row, c) * c_prop * acc;  dx0[row] (+)= alpha * dh[row] (+ dx[row] when dx is null: x and x_0 are one tensor)
template <bool BWD>
IA_DEV void gcn_row_finish(int row, int c, const f32x4& acc, const float* __restrict__ x, const float* __restrict__ x0, float* __restrict__ out,
                           float* __restrict__ out0, int acc0, int C, float c_prop, float alpha, const GcnDrop& d) {
  const size_t o = (size_t)row * C + c;
  if (!BWD) {
    const f32x4 r = ld4(x0 + o);
    f32x4 h;
#pragma unroll
    for (int e = 0; e < 4; ++e) h[e] = fmaf(c_prop, acc[e], alpha * r[e]);
    st4(out + o, h);
  } else {
    const f32x4 keep = gcn_keep4(d, (uint32_t)row * (uint32_t)C + (uint32_t)c, c_prop);
    const f32x4 g = acc * keep;
    if (out) st4(out + o, g);
    if (out0) {
      const f32x4 dh = ld4(x + o);
      f32x4 r = acc0 ? ld4(out0 + o) : zero4();
#pragma unroll
      for (int e = 0; e < 4; ++e) r[e] = fmaf(alpha, dh[e], r[e]);
      if (!out) r += g;
      st4(out0 + o, r);
    }
  }
}

template <bool HALF, bool COL64, bool BWD>
__global__ __launch_bounds__(1024) void gcn_propagate_kernel(const int64_t* __restrict__ rowptr, const void* __restrict__ col,
                                                             const float* __restrict__ val, const float* __restrict__ x,
                                                             const float* __restrict__ x0, float* __restrict__ out, float* __restrict__ out0,
                                                             int acc0, int N, int C, float c_prop, float alpha, GcnDrop d,
                                                             const int32_t* __restrict__ long_rows, int n_long) {
  __shared__ f32x4 s_part[GCN_WAVES][GCN_MAXC / 4];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const bool owner = HALF ? lane < 32 : true;
  const int c0 = HALF ? (lane & 31) * 4 : lane * 4;
  f32x4 acc[2];
  if ((int)blockIdx.x >= n_long) {                       // 16 short rows, one per wave
    const long row = ((long)blockIdx.x - n_long) * GCN_WAVES + wave;
    if (row >= N) return;
    const long lo = rowptr[row], hi = rowptr[row + 1];
    if (long_rows && hi - lo > GCN_LONG) return;         // done by the workgroup that long_rows gives it to
    gcn_row_sum<HALF, COL64, BWD>(col, val, x, lo, hi, N, C, d, lane, acc);
    if (owner) {
#pragma unroll
      for (int k = 0; k < (HALF ? 1 : 2); ++k)
        if (c0 + 256 * k < C) gcn_row_finish<BWD>((int)row, c0 + 256 * k, acc[k], x, x0, out, out0, acc0, C, c_prop, alpha, d);
    }
    return;
  }
  const int row = long_rows[blockIdx.x];                 // one long row: 16 contiguous chunks, joined in chunk order
  if (row < 0 || row >= N) return;
  const long lo = rowptr[row], hi = rowptr[row + 1];
  if (hi - lo <= GCN_LONG) return;                       // a short row in the list stays with the short path
  long chunk = (hi - lo + GCN_WAVES - 1) / GCN_WAVES;
  chunk += chunk & 1;
  const long wlo = min(hi, lo + wave * chunk), whi = min(hi, wlo + chunk);
  gcn_row_sum<HALF, COL64, BWD>(col, val, x, wlo, whi, N, C, d, lane, acc);
  if (owner) {
#pragma unroll
    for (int k = 0; k < (HALF ? 1 : 2); ++k)
      if (c0 + 256 * k < C) s_part[wave][(c0 + 256 * k) >> 2] = acc[k];
  }
  __syncthreads();
  const int c = threadIdx.x * 4;
  if (c < C) {
    f32x4 s = s_part[0][threadIdx.x];
    for (int w = 1; w < GCN_WAVES; ++w) s += s_part[w][threadIdx.x];
    gcn_row_finish<BWD>(row, c, s, x, x0, out, out0, acc0, C, c_prop, alpha, d);
  }
}

// ------------------------------------------------------------------------------------------------ tall-skinny products
// Operand forms: a plain matrix, a matrix under dropout, or the gradient in front of a relu taken from the gradient behind it and
// the relu's (possibly dropped) output: g * (y > 0 ? gscale : 0).
enum { GA_PLAIN = 0, GA_DROP = 1, GA_RELUGRAD = 2 };
enum { GE_MIX = 0, GE_BIAS_RELU = 1, GE_MIXBWD = 2 };

template <int MODE>
IA_DEV f32x4 gcn_operand4(const float* __restrict__ A, const float* __restrict__ A2, size_t o, float gscale, const GcnDrop& d) {
  f32x4 v = ld4(A + o);
  if (MODE == GA_DROP) v = v * gcn_keep4(d, (uint32_t)o, d.inv_keep);
  if (MODE == GA_RELUGRAD) {
    const f32x4 y = ld4(A2 + o);
#pragma unroll
    for (int e = 0; e < 4; ++e) v[e] = y[e] > 0.f ? v[e] * gscale : 0.f;
  }
  return v;
}

constexpr int GBM = 128, GBN = 64, GBK = 16;

// C[m][n] = epilogue(sum_k A'(m, k) B[k sbk + n sbn]), k ascending (one fmaf chain per output); A' row-major [M, K] in form AMODE.
//   GE_MIX:       relu((1 - beta) A[m][n] + beta acc), then the output dropout `dout`         (K == Nc)
//   GE_BIAS_RELU: relu(acc + bias[n])
//   GE_MIXBWD:    (1 - beta) A'(m, n) + beta acc                                                (K == Nc)
template <int AMODE, int EPI>
__global__ __launch_bounds__(256) void gcn_rows_gemm_kernel(const float* __restrict__ A, const float* __restrict__ A2, int lda,
                                                            const float* __restrict__ Bm, long sbk, long sbn, const float* __restrict__ bias,
                                                            float* __restrict__ Cm, int ldc, int M, int Nc, int K, float beta, float gscale,
                                                            GcnDrop din, GcnDrop dout) {
  __shared__ float As[GBK][GBM + 4];
  __shared__ float Bs[GBK][GBN + 4];
  const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
  const int m0 = blockIdx.y * GBM, n0 = blockIdx.x * GBN;
  float acc[8][4] = {};
  for (int k0 = 0; k0 < K; k0 += GBK) {
#pragma unroll
    for (int q = 0; q < 2; ++q) {
      const int idx = tid + 256 * q, mm = idx >> 2, k4 = (idx & 3) * 4;
      const int gm = m0 + mm, gk = k0 + k4;
      f32x4 v = zero4();
      if (gm < M && gk < K) v = gcn_operand4<AMODE>(A, A2, (size_t)gm * lda + gk, gscale, din);
#pragma unroll
      for (int e = 0; e < 4; ++e) As[k4 + e][mm] = v[e];
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int e = tid + 256 * q;
      int nn, kk;
      if (sbk == 1) { nn = e >> 4; kk = e & 15; } else { kk = e >> 6; nn = e & 63; }
      const int gn = n0 + nn, gk = k0 + kk;
      Bs[kk][nn] = (gn < Nc && gk < K) ? Bm[gk * sbk + gn * sbn] : 0.f;
    }
    __syncthreads();
#pragma unroll
    for (int kk = 0; kk < GBK; ++kk) {
      const f32x4 a0 = ld4(&As[kk][ty * 8]), a1 = ld4(&As[kk][ty * 8 + 4]);
      const f32x4 b = ld4(&Bs[kk][tx * 4]);
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          acc[i][j] = fmaf(a0[i], b[j], acc[i][j]);
          acc[4 + i][j] = fmaf(a1[i], b[j], acc[4 + i][j]);
        }
    }
    __syncthreads();
  }
  const int gn = n0 + tx * 4;
  if (gn >= Nc) return;
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const int gm = m0 + ty * 8 + i;
    if (gm >= M) continue;
    f32x4 v = {acc[i][0], acc[i][1], acc[i][2], acc[i][3]};
    if (EPI == GE_MIX) {
      const f32x4 h = ld4(A + (size_t)gm * lda + gn);
#pragma unroll
      for (int e = 0; e < 4; ++e) v[e] = fmaxf(fmaf(beta, v[e], (1.f - beta) * h[e]), 0.f);
      if (dout.thr16) v = v * gcn_keep4(dout, (uint32_t)((size_t)gm * ldc + gn), dout.inv_keep);
    } else if (EPI == GE_BIAS_RELU) {
      const f32x4 b = ld4(bias + gn);
#pragma unroll
      for (int e = 0; e < 4; ++e) v[e] = fmaxf(v[e] + b[e], 0.f);
    } else {
      const f32x4 g = gcn_operand4<AMODE>(A, A2, (size_t)gm * lda + gn, gscale, din);
#pragma unroll
      for (int e = 0; e < 4; ++e) v[e] = fmaf(beta, v[e], (1.f - beta) * g[e]);
    }
    st4(Cm + (size_t)gm * ldc + gn, v);
  }
}

// part[z][m][n] = sum over the node rows r of slab z (ascending) of P'(r, m) Q'(r, n);  csum[z][m] = sum_r P'(r, m)   (CSUM)
template <int PMODE, int QMODE, bool CSUM>
__global__ __launch_bounds__(256) void gcn_tn_gemm_kernel(const float* __restrict__ P, const float* __restrict__ P2, int ldp,
                                                          const float* __restrict__ Q, const float* __restrict__ Q2, int ldq,
                                                          float* __restrict__ part, float* __restrict__ csum, int Mo, int No, int rows,
                                                          float gscale, GcnDrop dq) {
  __shared__ float As[GBK][GBM + 4];
  __shared__ float Bs[GBK][GBN + 4];
  const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
  const int m0 = blockIdx.y * GBM, n0 = blockIdx.x * GBN;
  const int r_lo = blockIdx.z * GCN_SLAB, r_hi = min(rows, r_lo + GCN_SLAB);
  float acc[8][4] = {};
  float rsum[8] = {};
  const GcnDrop none{0u, 1.f, 0u, 0u};
  for (int r0 = r_lo; r0 < r_hi; r0 += GBK) {
#pragma unroll
    for (int q = 0; q < 2; ++q) {
      const int idx = tid + 256 * q, kk = idx >> 5, m4 = (idx & 31) * 4;
      const int r = r0 + kk, gm = m0 + m4;
      f32x4 v = zero4();
      if (r < r_hi && gm < Mo) v = gcn_operand4<PMODE>(P, P2, (size_t)r * ldp + gm, gscale, none);
      st4(&As[kk][m4], v);
    }
    {
      const int kk = tid >> 4, n4 = (tid & 15) * 4;
      const int r = r0 + kk, gn = n0 + n4;
      f32x4 v = zero4();
      if (r < r_hi && gn < No) v = gcn_operand4<QMODE>(Q, Q2, (size_t)r * ldq + gn, gscale, dq);
      st4(&Bs[kk][n4], v);
    }
    __syncthreads();
#pragma unroll
    for (int kk = 0; kk < GBK; ++kk) {
      const f32x4 a0 = ld4(&As[kk][ty * 8]), a1 = ld4(&As[kk][ty * 8 + 4]);
      const f32x4 b = ld4(&Bs[kk][tx * 4]);
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        if (CSUM) { rsum[i] += a0[i]; rsum[4 + i] += a1[i]; }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          acc[i][j] = fmaf(a0[i], b[j], acc[i][j]);
          acc[4 + i][j] = fmaf(a1[i], b[j], acc[4 + i][j]);
        }
      }
    }
    __syncthreads();
  }
  float* pz = part + (size_t)blockIdx.z * Mo * No;
  const int gn = n0 + tx * 4;
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const int gm = m0 + ty * 8 + i;
    if (gm >= Mo) continue;
    if (gn < No) st4(pz + (size_t)gm * No + gn, f32x4{acc[i][0], acc[i][1], acc[i][2], acc[i][3]});
    if (CSUM && blockIdx.x == 0 && tx == 0) csum[(size_t)blockIdx.z * Mo + gm] = rsum[i];
  }
}

// dst[i] += scale * sum_z part[z][i], z ascending, summed in fp64 and rounded once
__global__ __launch_bounds__(256) void gcn_slab_sum_kernel(const float* __restrict__ part, float* __restrict__ dst, size_t n, int S, float scale) {
  for (size_t i = blockIdx.x * 256ull + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) {
    double s = 0.0;
    for (int z = 0; z < S; ++z) s += (double)part[(size_t)z * n + i];
    dst[i] += scale * (float)s;
  }
}

// ------------------------------------------------------------------------------------------------ pair stage
__global__ __launch_bounds__(256) void gcn_pair_gather_kernel(const float* __restrict__ x, const int32_t* __restrict__ idx, float* __restrict__ out,
                                                              int R, int C, int N, GcnDrop d) {
  const int t = blockIdx.x * 256 + threadIdx.x, c4 = C >> 2;
  if (t >= R * c4) return;
  const int r = t / c4, c = (t % c4) * 4;
  const int node = idx[r];
  f32x4 v = (node >= 0 && node < N) ? ld4(x + (size_t)node * C + c) : zero4();
  v = v * gcn_keep4(d, (uint32_t)r * (uint32_t)C + (uint32_t)c, d.inv_keep);
  st4(out + (size_t)r * C + c, v);
}

// order = the pair rows stably sorted by node: the thread at the first position of a run of equal nodes adds the run up in that
// order and is the only writer of the node's row
__global__ __launch_bounds__(256) void gcn_pair_scatter_kernel(const float* __restrict__ dout, const int32_t* __restrict__ idx,
                                                               const int32_t* __restrict__ order, float* __restrict__ dnode, int R, int C, int N,
                                                               GcnDrop d) {
  const int t = blockIdx.x * 256 + threadIdx.x, c4 = C >> 2;
  if (t >= R * c4) return;
  const int s = t / c4, c = (t % c4) * 4;
  auto node_at = [&](int pos) -> int {
    const int r = order[pos];
    return (r >= 0 && r < R) ? idx[r] : -1;
  };
  const int node = node_at(s);
  if (node < 0 || node >= N) return;
  if (s > 0 && node_at(s - 1) == node) return;
  f32x4 acc = zero4();
  for (int q = s; q < R && node_at(q) == node; ++q) {
    const int r = order[q];
    acc += ld4(dout + (size_t)r * C + c) * gcn_keep4(d, (uint32_t)r * (uint32_t)C + (uint32_t)c, d.inv_keep);
  }
  float* p = dnode + (size_t)node * C + c;
  st4(p, ld4(p) + acc);
}

// ------------------------------------------------------------------------------------------------ host side
bool gcn_aligned(const void* p) { return ((uintptr_t)p & 15) == 0; }
bool gcn_width_ok(int C) { return C >= 32 && C <= GCN_MAXC && C % 32 == 0; }
bool gcn_size_ok(int N, int W) { return N > 0 && W > 0 && (uint64_t)N * (uint64_t)W < (1ull << 32); }
bool gcn_drop_ok(float p) { return p >= 0.f && p < 1.f; }
int gcn_slabs(int N) { return (N + GCN_SLAB - 1) / GCN_SLAB; }

template <bool BWD>
int gcn_propagate(const int64_t* rowptr, const void* col, int col_is_64, const float* val, const float* x, const float* x0, float* out,
                  float* out0, int acc0, int N, int C, float alpha, float drop_p, uint32_t seed, uint32_t stream_id,
                  const int32_t* long_rows, int n_long, hipStream_t stream) {
  const GcnDrop d = gcn_drop(drop_p, seed, stream_id);
  const float c_prop = (1.f - alpha) * d.inv_keep;
  if (!long_rows) n_long = 0;
  const dim3 grid((unsigned)(n_long + (N + GCN_WAVES - 1) / GCN_WAVES)), blk(64 * GCN_WAVES);
#define IA_P(HALF, COL64) hipLaunchKernelGGL((gcn_propagate_kernel<HALF, COL64, BWD>), grid, blk, 0, stream, rowptr, col, val, x, x0, out, out0, \
    acc0, N, C, c_prop, alpha, d, long_rows, n_long)
  if (C <= 128) { if (col_is_64) IA_P(true, true); else IA_P(true, false); }
  else { if (col_is_64) IA_P(false, true); else IA_P(false, false); }
#undef IA_P
  return ia_check_launch();
}

}  // namespace

extern "C" int ia_gcn_propagate_fwd(const int64_t* rowptr, const void* col, int col_is_64, const float* val, const float* x, const float* x0,
                                    float* h, int N, int C, float alpha, float drop_p, uint32_t seed, uint32_t stream_id,
                                    const int32_t* long_rows, int n_long, hipStream_t stream) {
  (void)hipGetLastError();
  if (!rowptr || !col || !x || !x0 || !h || !gcn_width_ok(C) || !gcn_size_ok(N, C) || !gcn_drop_ok(drop_p) || n_long < 0) return IA_ERR_ARG;
  if (!gcn_aligned(x) || !gcn_aligned(x0) || !gcn_aligned(h) || h == x || h == x0) return IA_ERR_ARG;
  return gcn_propagate<false>(rowptr, col, col_is_64, val, x, x0, h, nullptr, 0, N, C, alpha, drop_p, seed, stream_id, long_rows, n_long, stream);
}

extern "C" int ia_gcn_propagate_bwd(const int64_t* rowptr_t, const void* col_t, int col_is_64, const float* val_t, const float* dh, float* dx,
                                    float* dx0, int dx0_accumulate, int N, int C, float alpha, float drop_p, uint32_t seed, uint32_t stream_id,
                                    const int32_t* long_rows_t, int n_long_t, hipStream_t stream) {
  (void)hipGetLastError();
  if (!rowptr_t || !col_t || !dh || (!dx && !dx0) || !gcn_width_ok(C) || !gcn_size_ok(N, C) || !gcn_drop_ok(drop_p) || n_long_t < 0)
    return IA_ERR_ARG;
  if (!gcn_aligned(dh) || !gcn_aligned(dx) || !gcn_aligned(dx0) || dx == dh || dx0 == dh) return IA_ERR_ARG;
  return gcn_propagate<true>(rowptr_t, col_t, col_is_64, val_t, dh, nullptr, dx, dx0, dx0_accumulate, N, C, alpha, drop_p, seed, stream_id,
                             long_rows_t, n_long_t, stream);
}

extern "C" int ia_gcn_mix_fwd(const float* h, const float* W, float* out, int N, int C, float beta, float drop_p, uint32_t seed,
                              uint32_t stream_id, hipStream_t stream) {
  (void)hipGetLastError();
  if (!h || !W || !out || out == h || !gcn_width_ok(C) || !gcn_size_ok(N, C) || !gcn_drop_ok(drop_p)) return IA_ERR_ARG;
  if (!gcn_aligned(h) || !gcn_aligned(out)) return IA_ERR_ARG;
  const GcnDrop none = gcn_drop(0.f, 0, 0), d = gcn_drop(drop_p, seed, stream_id);
  const dim3 grid((C + GBN - 1) / GBN, (N + GBM - 1) / GBM);
  hipLaunchKernelGGL((gcn_rows_gemm_kernel<GA_PLAIN, GE_MIX>), grid, dim3(256), 0, stream, h, (const float*)nullptr, C, W, (long)C, 1L,
                     (const float*)nullptr, out, C, N, C, C, beta, 1.f, none, d);
  return ia_check_launch();
}

extern "C" size_t ia_gcn_workspace_bytes(int N, int C, int F) {
  if (N <= 0 || C <= 0 || F < 0) return 0;
  const size_t wide = (size_t)(F > C ? F : C);
  return (size_t)gcn_slabs(N) * ((size_t)C * wide + (size_t)C) * sizeof(float);
}

extern "C" int ia_gcn_mix_bwd(const float* dout, const float* out, const float* h, const float* W, float* dh, float* dW, int N, int C, float beta,
                              float drop_p, void* workspace, size_t workspace_bytes, hipStream_t stream) {
  (void)hipGetLastError();
  if (!dout || !out || !h || !W || !dh || dh == dout || dh == out || dh == h || !gcn_width_ok(C) || !gcn_size_ok(N, C) || !gcn_drop_ok(drop_p))
    return IA_ERR_ARG;
  if (!gcn_aligned(dout) || !gcn_aligned(out) || !gcn_aligned(h) || !gcn_aligned(dh) || !gcn_aligned(workspace)) return IA_ERR_ARG;
  if (dW && (!workspace || workspace_bytes < ia_gcn_workspace_bytes(N, C, 0))) return IA_ERR_WORKSPACE;
  const GcnDrop none = gcn_drop(0.f, 0, 0);
  const float gscale = gcn_drop(drop_p, 0, 0).inv_keep;
  // dh = (1 - beta) dpre + beta dpre W^T
  const dim3 grid((C + GBN - 1) / GBN, (N + GBM - 1) / GBM);
  hipLaunchKernelGGL((gcn_rows_gemm_kernel<GA_RELUGRAD, GE_MIXBWD>), grid, dim3(256), 0, stream, dout, out, C, W, 1L, (long)C,
                     (const float*)nullptr, dh, C, N, C, C, beta, gscale, none, none);
  if (dW) {   // dW += beta h^T dpre
    const int S = gcn_slabs(N);
    float* part = (float*)workspace;
    const dim3 tgrid((C + GBN - 1) / GBN, (C + GBM - 1) / GBM, S);
    hipLaunchKernelGGL((gcn_tn_gemm_kernel<GA_PLAIN, GA_RELUGRAD, false>), tgrid, dim3(256), 0, stream, h, (const float*)nullptr, C, dout, out, C,
                       part, (float*)nullptr, C, C, N, gscale, none);
    hipLaunchKernelGGL(gcn_slab_sum_kernel, dim3((C * C + 255) / 256), dim3(256), 0, stream, part, dW, (size_t)C * C, S, beta);
  }
  return ia_check_launch();
}

extern "C" int ia_gcn_input_fwd(const float* X, const float* W, const float* bias, float* x0, int N, int F, int C, float drop_p, uint32_t seed,
                                uint32_t stream_id, hipStream_t stream) {
  (void)hipGetLastError();
  if (!X || !W || !bias || !x0 || !gcn_width_ok(C) || F <= 0 || (F & 3) || !gcn_size_ok(N, F) || !gcn_size_ok(N, C) || !gcn_drop_ok(drop_p))
    return IA_ERR_ARG;
  if (!gcn_aligned(X) || !gcn_aligned(x0) || !gcn_aligned(bias)) return IA_ERR_ARG;
  const GcnDrop none = gcn_drop(0.f, 0, 0), d = gcn_drop(drop_p, seed, stream_id);
  const dim3 grid((C + GBN - 1) / GBN, (N + GBM - 1) / GBM);
  if (d.thr16)
    hipLaunchKernelGGL((gcn_rows_gemm_kernel<GA_DROP, GE_BIAS_RELU>), grid, dim3(256), 0, stream, X, (const float*)nullptr, F, W, 1L, (long)F, bias,
                       x0, C, N, C, F, 0.f, 1.f, d, none);
  else
    hipLaunchKernelGGL((gcn_rows_gemm_kernel<GA_PLAIN, GE_BIAS_RELU>), grid, dim3(256), 0, stream, X, (const float*)nullptr, F, W, 1L, (long)F, bias,
                       x0, C, N, C, F, 0.f, 1.f, none, none);
  return ia_check_launch();
}

extern "C" int ia_gcn_input_bwd(const float* dx0, const float* x0, const float* X, float* dW, float* db, int N, int F, int C, float drop_p,
                                uint32_t seed, uint32_t stream_id, void* workspace, size_t workspace_bytes, hipStream_t stream) {
  (void)hipGetLastError();
  if (!dx0 || !x0 || !X || !dW || !db || !gcn_width_ok(C) || F <= 0 || (F & 3) || !gcn_size_ok(N, F) || !gcn_size_ok(N, C) || !gcn_drop_ok(drop_p))
    return IA_ERR_ARG;
  if (!gcn_aligned(dx0) || !gcn_aligned(x0) || !gcn_aligned(X) || !gcn_aligned(workspace)) return IA_ERR_ARG;
  if (!workspace || workspace_bytes < ia_gcn_workspace_bytes(N, C, F)) return IA_ERR_WORKSPACE;
  const GcnDrop d = gcn_drop(drop_p, seed, stream_id);
  const int S = gcn_slabs(N);
  float* part = (float*)workspace;
  float* csum = part + (size_t)S * C * F;
  const dim3 tgrid((F + GBN - 1) / GBN, (C + GBM - 1) / GBM, S);
  if (d.thr16)
    hipLaunchKernelGGL((gcn_tn_gemm_kernel<GA_RELUGRAD, GA_DROP, true>), tgrid, dim3(256), 0, stream, dx0, x0, C, X, (const float*)nullptr, F, part,
                       csum, C, F, N, 1.f, d);
  else
    hipLaunchKernelGGL((gcn_tn_gemm_kernel<GA_RELUGRAD, GA_PLAIN, true>), tgrid, dim3(256), 0, stream, dx0, x0, C, X, (const float*)nullptr, F, part,
                       csum, C, F, N, 1.f, d);
  hipLaunchKernelGGL(gcn_slab_sum_kernel, dim3((unsigned)(((size_t)C * F + 255) / 256)), dim3(256), 0, stream, part, dW, (size_t)C * F, S, 1.f);
  hipLaunchKernelGGL(gcn_slab_sum_kernel, dim3((C + 255) / 256), dim3(256), 0, stream, csum, db, (size_t)C, S, 1.f);
  return ia_check_launch();
}

extern "C" int ia_gcn_pair_gather_fwd(const float* x, const int32_t* idx, float* out, int R, int C, int N, float drop_p, uint32_t seed,
                                      uint32_t stream_id, hipStream_t stream) {
  (void)hipGetLastError();
  if (!x || !idx || !out || R <= 0 || !gcn_width_ok(C) || !gcn_size_ok(N, C) || !gcn_size_ok(R, C) || !gcn_drop_ok(drop_p)) return IA_ERR_ARG;
  if (!gcn_aligned(x) || !gcn_aligned(out)) return IA_ERR_ARG;
  hipLaunchKernelGGL(gcn_pair_gather_kernel, dim3((R * (C / 4) + 255) / 256), dim3(256), 0, stream, x, idx, out, R, C, N,
                     gcn_drop(drop_p, seed, stream_id));
  return ia_check_launch();
}

extern "C" int ia_gcn_pair_scatter_bwd(const float* dout, const int32_t* idx, const int32_t* order, float* dnode, int R, int C, int N, float drop_p,
                                       uint32_t seed, uint32_t stream_id, hipStream_t stream) {
  (void)hipGetLastError();
  if (!dout || !idx || !order || !dnode || R <= 0 || !gcn_width_ok(C) || !gcn_size_ok(N, C) || !gcn_size_ok(R, C) || !gcn_drop_ok(drop_p))
    return IA_ERR_ARG;
  if (!gcn_aligned(dout) || !gcn_aligned(dnode)) return IA_ERR_ARG;
  hipLaunchKernelGGL(gcn_pair_scatter_kernel, dim3((R * (C / 4) + 255) / 256), dim3(256), 0, stream, dout, idx, order, dnode, R, C, N,
                     gcn_drop(drop_p, seed, stream_id));
  return ia_check_launch();
}
