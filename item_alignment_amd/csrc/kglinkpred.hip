// Link-prediction ranks of the PKGM / TransE tables (reference pkgm_pretrain.py --do_test over the vendored torchkge:
// evaluation.py LinkPredictionEvaluator, utils/modeling.py filter_scores, utils/operations.py get_rank).  No [B, n_ent] score matrix:
// the candidate table streams through LDS tiles and only the counts leave the kernel.
//
// One ia_kgpt_lp_rank call ranks B queries on one side:
//   tail side: q = ent[h] + rel[r], true entity t;   head side: q = ent[t] - rel[r], true entity h
//   d(q, c) = sum_k |q_k - c_k|^2 (norm 2) or sum_k |q_k - c_k| (norm 1), score = -d; raw rank = 1 + #{c != true : d_c <= d_true}
//   1. prep:    q rows into the workspace (one wave per query); ids out of range mark the query dead (rank 0)
//   2. true:    d_true of every query in the listed-candidates mode (lp_dist over the one id)
//   3. scan:    every (query, candidate) pair of a 128 x 128 tile from LDS, 8 x 8 pairs per thread in packed f32; the counts
//               of d_c <= d_true are summed per workgroup in LDS and added to the query's global count with one integer atomic
//   4. filter:  lp_dist over the query's filter group (CSR), true id skipped: the members the scan counted, subtracted
//   5. finish:  rank = 1 + count, filt_rank = rank - filtered count (int64)
// Every pair's d is one fp32 accumulator summed in k order 0 .. D-1 through lp_step (the zero padding past D adds +0, an identity),
// so the scan and the listed mode produce the same bits for the same pair and the true entity counts itself exactly once.
#include "common.h"
#include "../../include/itemalign.h"
#include "kgpair.h"   // lp_step, lp_dist and the tile constants (shared with kgtopk.hip)

namespace {

// ------------------------------------------------------------------------------------------------ 1. query rows
__global__ __launch_bounds__(256) void lp_prep_kernel(const float* __restrict__ ent, const float* __restrict__ rel, const int64_t* __restrict__ h,
                                                      const int64_t* __restrict__ t, const int64_t* __restrict__ r, int B, int D, int n_ent,
                                                      int n_rel, int side, float* __restrict__ q, int64_t* __restrict__ tru) {
  const int b = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (b >= B) return;                                          // wave-uniform
  const int64_t hh = h[b], tt = t[b], rr = r[b];
  const bool ok = hh >= 0 && hh < n_ent && tt >= 0 && tt < n_ent && rr >= 0 && rr < n_rel;
  const bool tail = side == IA_KGPT_LP_TAIL;
  const float* a = ent + (ok ? (size_t)(tail ? hh : tt) * D : 0);
  const float* rv = rel + (ok ? (size_t)rr * D : 0);
  float* dst = q + (size_t)b * D;
  for (int c = lane * 4; c < D; c += 256) {
    f32x4 v = {0.f, 0.f, 0.f, 0.f};
    if (ok) {
      const f32x4 x = *reinterpret_cast<const f32x4*>(a + c), y = *reinterpret_cast<const f32x4*>(rv + c);
      v = tail ? x + y : x - y;
    }
    *reinterpret_cast<f32x4*>(dst + c) = v;
  }
  if (lane == 0) tru[b] = ok ? (tail ? tt : hh) : -1;
}

// ------------------------------------------------------------------------------------------------ 2. true distances
template <int NORM>
__global__ __launch_bounds__(256) void lp_true_kernel(const float* __restrict__ ent, const float* __restrict__ q, const int64_t* __restrict__ tru,
                                                      int B, int D, float* __restrict__ dtrue) {
  const int b = blockIdx.x * 256 + threadIdx.x;
  if (b >= B) return;
  const int64_t e = tru[b];
  dtrue[b] = e >= 0 ? lp_dist<NORM>(q + (size_t)b * D, ent + (size_t)e * D, D) : 0.f;
}

// ------------------------------------------------------------------------------------------------ 3. full scan
// Workgroup (x, y): queries [128 (qt0 + y), + 128), candidate tiles [x tps, x tps + tps) (the host walks qt0 past grid y's 65535 cap).  Thread (tx, ty) = (tid & 15, tid >> 4)
// owns queries ty*4 + {0..3} and 64 + ty*4 + {0..3}, candidates tx*4 + {0..3} and 64 + tx*4 + {0..3} of the tile: each LDS read is
// one ds_read_b128 over 16 contiguous lanes' slots.  STORE: also scores[b, c] = -d (the bits the comparison used).
IA_DEV int lp_row(int i) { return (i & 3) + ((i >> 2) << 6); }   // i in [0, 8) -> offset of the i-th owned row (add 4 * tx / 4 * ty)

template <int NORM, bool STORE>
__global__ __launch_bounds__(256) void lp_scan_kernel(const float* __restrict__ ent, const float* __restrict__ q, const int64_t* __restrict__ tru,
                                                      const float* __restrict__ dtrue, int B, int D, int n_ent, int tiles_per_split,
                                                      int qt0, int* __restrict__ cnt, float* __restrict__ scores) {
  __shared__ float Qs[LP_DK][LP_LD];
  __shared__ float Cs[LP_DK][LP_LD];
  __shared__ int s_cnt[LP_QT];
  const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
  const int q0 = (qt0 + (int)blockIdx.y) * LP_QT;
  const int n_tiles = (n_ent + LP_CT - 1) / LP_CT;
  const int ct_lo = blockIdx.x * tiles_per_split, ct_hi = min(n_tiles, ct_lo + tiles_per_split);
  if (tid < LP_QT) s_cnt[tid] = 0;
  int64_t my_true[8];
  float my_dtrue[8];
  int my_cnt[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const int b = q0 + ty * 4 + lp_row(i);
    my_true[i] = b < B ? tru[b] : -1;
    my_dtrue[i] = b < B ? dtrue[b] : 0.f;
    my_cnt[i] = 0;
  }
  for (int ct = ct_lo; ct < ct_hi; ++ct) {
    const int c0 = ct * LP_CT;
    f32x2 acc[8][4];
#pragma unroll
    for (int i = 0; i < 8; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j) acc[i][j] = f32x2{0.f, 0.f};
    for (int k0 = 0; k0 < D; k0 += LP_DK) {
      f32x4 vq[2], vc[2];
#pragma unroll
      for (int s = 0; s < 2; ++s) {
        const int e = tid + 256 * s, row = e >> 2, kk = (e & 3) * 4, k = k0 + kk;
        const int gq = q0 + row, gc = c0 + row;
        vq[s] = (gq < B && k < D) ? *reinterpret_cast<const f32x4*>(q + (size_t)gq * D + k) : f32x4{0.f, 0.f, 0.f, 0.f};
        vc[s] = (gc < n_ent && k < D) ? *reinterpret_cast<const f32x4*>(ent + (size_t)gc * D + k) : f32x4{0.f, 0.f, 0.f, 0.f};
      }
      __syncthreads();                                       // the previous stage's reads are done
#pragma unroll
      for (int s = 0; s < 2; ++s) {
        const int e = tid + 256 * s, row = e >> 2, kk = (e & 3) * 4;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          Qs[kk + i][row] = vq[s][i];
          Cs[kk + i][row] = vc[s][i];
        }
      }
      __syncthreads();
#pragma unroll
      for (int kk = 0; kk < LP_DK; ++kk) {
        const f32x4 a0 = *reinterpret_cast<const f32x4*>(&Qs[kk][ty * 4]), a1 = *reinterpret_cast<const f32x4*>(&Qs[kk][64 + ty * 4]);
        const f32x4 c0v = *reinterpret_cast<const f32x4*>(&Cs[kk][tx * 4]), c1v = *reinterpret_cast<const f32x4*>(&Cs[kk][64 + tx * 4]);
        const f32x2 cp[4] = {f32x2{c0v[0], c0v[1]}, f32x2{c0v[2], c0v[3]}, f32x2{c1v[0], c1v[1]}, f32x2{c1v[2], c1v[3]}};
#pragma unroll
        for (int i = 0; i < 8; ++i) {
          const float qa = i < 4 ? a0[i] : a1[i - 4];
          const f32x2 qq = {qa, qa};
#pragma unroll
          for (int j = 0; j < 4; ++j) acc[i][j] = lp_step<NORM>(acc[i][j], qq, cp[j]);
        }
      }
    }
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const int b = q0 + ty * 4 + lp_row(i);
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const int c = c0 + tx * 4 + lp_row(j);
        const float d = acc[i][j >> 1][j & 1];
        my_cnt[i] += (c < n_ent && (int64_t)c != my_true[i] && d <= my_dtrue[i]) ? 1 : 0;
        if (STORE && b < B && c < n_ent) scores[(size_t)b * n_ent + c] = -d;
      }
    }
  }
  __syncthreads();
#pragma unroll
  for (int i = 0; i < 8; ++i)
    if (my_cnt[i]) atomicAdd(&s_cnt[ty * 4 + lp_row(i)], my_cnt[i]);
  __syncthreads();
  if (tid < LP_QT && q0 + tid < B && s_cnt[tid]) atomicAdd(&cnt[q0 + tid], s_cnt[tid]);
}

// ------------------------------------------------------------------------------------------------ 4. filter correction
// One workgroup per query: the members of its group (sorted, unique ids) other than the true id with d <= d_true
template <int NORM>
__global__ __launch_bounds__(256) void lp_filter_kernel(const float* __restrict__ ent, const float* __restrict__ q, const int64_t* __restrict__ tru,
                                                        const float* __restrict__ dtrue, const int64_t* __restrict__ grp_off,
                                                        const int64_t* __restrict__ grp_ids, int n_grp, const int64_t* __restrict__ q_grp,
                                                        int D, int n_ent, int* __restrict__ fcnt) {
  __shared__ int s[4];
  const int b = blockIdx.x;
  const int64_t e = tru[b];
  const int64_t g = q_grp[b];
  int n = 0;
  if (e >= 0 && g >= 0 && g < n_grp) {
    const float* qb = q + (size_t)b * D;
    const float dt = dtrue[b];
    for (int64_t i = grp_off[g] + threadIdx.x; i < grp_off[g + 1]; i += 256) {
      const int64_t c = grp_ids[i];
      if (c < 0 || c >= n_ent || c == e) continue;
      n += lp_dist<NORM>(qb, ent + (size_t)c * D, D) <= dt ? 1 : 0;
    }
  }
  for (int o = 32; o > 0; o >>= 1) n += __shfl_xor(n, o);
  if ((threadIdx.x & 63) == 0) s[threadIdx.x >> 6] = n;
  __syncthreads();
  if (threadIdx.x == 0) fcnt[b] = s[0] + s[1] + s[2] + s[3];
}

// ------------------------------------------------------------------------------------------------ 5. ranks
__global__ __launch_bounds__(256) void lp_finish_kernel(const int64_t* __restrict__ tru, const int* __restrict__ cnt, const int* __restrict__ fcnt,
                                                        int B, int filtered, int64_t* __restrict__ rank, int64_t* __restrict__ filt_rank) {
  const int b = blockIdx.x * 256 + threadIdx.x;
  if (b >= B) return;
  const bool ok = tru[b] >= 0;
  const int64_t rk = ok ? 1 + (int64_t)cnt[b] : 0;
  rank[b] = rk;
  filt_rank[b] = ok ? rk - (filtered ? (int64_t)fcnt[b] : 0) : 0;
}

struct LpWs {
  float *q, *dtrue;
  int64_t* tru;
  int *cnt, *fcnt;
  size_t bytes;
};

LpWs lp_ws_layout(char* base, int B, int D) {
  LpWs w{};
  size_t off = 0;
  auto take = [&](size_t bytes) { char* p = base ? base + off : nullptr; off += (bytes + 255) / 256 * 256; return p; };
  w.q = reinterpret_cast<float*>(take((size_t)B * D * 4));
  w.dtrue = reinterpret_cast<float*>(take((size_t)B * 4));
  w.tru = reinterpret_cast<int64_t*>(take((size_t)B * 8));
  w.cnt = reinterpret_cast<int*>(take((size_t)B * 4));
  w.fcnt = reinterpret_cast<int*>(take((size_t)B * 4));
  w.bytes = off;
  return w;
}

}  // namespace

extern "C" size_t ia_kgpt_lp_workspace_bytes(int B, int D) {
  if (B <= 0 || D <= 0) return 0;
  return lp_ws_layout(nullptr, B, D).bytes;
}

extern "C" int ia_kgpt_lp_rank(const float* ent, const float* rel, const int64_t* h, const int64_t* t, const int64_t* r, int B, int D, int n_ent,
                               int n_rel, int norm, int side, const int64_t* grp_off, const int64_t* grp_ids, int n_grp, const int64_t* q_grp,
                               int64_t* rank, int64_t* filt_rank, float* scores, void* workspace, size_t workspace_bytes, hipStream_t stream) {
  (void)hipGetLastError();
  if (!ent || !rel || !h || !t || !r || !rank || !filt_rank) return IA_ERR_ARG;
  if (B <= 0 || D <= 0 || (D & 3) || n_ent <= 0 || n_rel <= 0 || (norm != 1 && norm != 2)) return IA_ERR_ARG;
  if (side != IA_KGPT_LP_TAIL && side != IA_KGPT_LP_HEAD) return IA_ERR_ARG;
  const int filtered = grp_off != nullptr;
  if (filtered && (!grp_ids || !q_grp || n_grp < 0)) return IA_ERR_ARG;
  if (!workspace || workspace_bytes < ia_kgpt_lp_workspace_bytes(B, D)) return IA_ERR_WORKSPACE;
  const LpWs w = lp_ws_layout((char*)workspace, B, D);
  const dim3 blk(256);
  if (hipMemsetAsync(w.cnt, 0, (size_t)B * 4, stream) != hipSuccess) return IA_ERR_LAUNCH;
  hipLaunchKernelGGL(lp_prep_kernel, dim3((B + 3) / 4), blk, 0, stream, ent, rel, h, t, r, B, D, n_ent, n_rel, side, w.q, w.tru);
  const int n_tiles = (n_ent + LP_CT - 1) / LP_CT, q_tiles = (B + LP_QT - 1) / LP_QT;
  int splits = (LP_TARGET_WGS + q_tiles - 1) / q_tiles;
  splits = splits < 1 ? 1 : (splits > n_tiles ? n_tiles : splits);
  const int tps = (n_tiles + splits - 1) / splits;
  splits = (n_tiles + tps - 1) / tps;
#define IA_LP(NORM)                                                                                                                        \
  hipLaunchKernelGGL(lp_true_kernel<NORM>, dim3((B + 255) / 256), blk, 0, stream, ent, w.q, w.tru, B, D, w.dtrue);                         \
  for (int qt0 = 0; qt0 < q_tiles; qt0 += LP_MAX_GRID_Y) {                                                                                \
    const dim3 sgrid(splits, min(LP_MAX_GRID_Y, q_tiles - qt0));                                                                           \
    if (scores)                                                                                                                            \
      hipLaunchKernelGGL((lp_scan_kernel<NORM, true>), sgrid, blk, 0, stream, ent, w.q, w.tru, w.dtrue, B, D, n_ent, tps, qt0, w.cnt, scores); \
    else                                                                                                                                   \
      hipLaunchKernelGGL((lp_scan_kernel<NORM, false>), sgrid, blk, 0, stream, ent, w.q, w.tru, w.dtrue, B, D, n_ent, tps, qt0, w.cnt,      \
                         scores);                                                                                                          \
  }                                                                                                                                        \
  if (filtered)                                                                                                                            \
    hipLaunchKernelGGL(lp_filter_kernel<NORM>, dim3(B), blk, 0, stream, ent, w.q, w.tru, w.dtrue, grp_off, grp_ids, n_grp, q_grp, D, n_ent, \
                       w.fcnt);
  if (norm == 2) { IA_LP(2) } else { IA_LP(1) }
#undef IA_LP
  hipLaunchKernelGGL(lp_finish_kernel, dim3((B + 255) / 256), blk, 0, stream, w.tru, w.cnt, w.fcnt, B, filtered, rank, filt_rank);
  return ia_check_launch();
}
