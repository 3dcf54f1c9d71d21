// Same-item retrieval: the k most similar catalogue rows of every query row, s(q, c) = sum_k q_k c_k (inner product; cosine on rows
// normalised by ia_sim_rows_bf16), without a [B, n_cand] score matrix.  A bf16 MFMA GEMM Q C^T whose epilogue is the streaming top-k
// of kgtopk.hip (topk_list.h).
//
//   1. ia_sim_rows_bf16: fp32 rows -> bf16 rows of `pitch` = D rounded up to ST_BK elements, the pad zero: the scan has no k tail
//   2. scan:  workgroup (query tile x, split y) walks its candidate tiles of ST_CT rows.  Four waves; wave w owns the queries
//             [32 NQ w, 32 NQ (w + 1)) of the tile and ALL candidates of it: NQ x 4 accumulators of mfma_f32_32x32x16_bf16 with the
//             candidates as the A operand (rows, in the 16 registers) and the queries as the B operand (columns, on the lane).  So
//             the 128 scores of a query within a tile sit in lanes l and l + 32 of one wave, and a query's list belongs to one wave:
//             insertions need no barrier.  Each pair has one accumulator that walks k in order whatever the split count (splits are
//             over candidates only): the score of a pair is a function of the two rows alone.
//             After a tile each score is tested in registers against the k-th best of its query (one compare per pair, plus the
//             range and skip tests); what passes is inserted by the whole wave into the query's sorted list in LDS.
//   3. merge: one wave per query folds the lists of the splits
// Key: an order-preserving map of the signed fp32 score, complemented (the smallest key is the best score), << 32 | candidate id:
// the unsigned order of the keys is (score descending, id ascending), keys are unique, so the k smallest do not depend on the
// arrival order of tiles or on the splits.
// NQ = 2 (256 queries a tile) while the lists fit beside it (k <= 32), NQ = 1 (128 queries) above: 256 x 64 keys would be 128 KiB.
#include "common.h"
#include "../../include/itemalign.h"
#include "topk_list.h"
#include "simscan.h"

namespace {

// ------------------------------------------------------------------------------------------------ 1. rows
// one wave per row
__global__ __launch_bounds__(256) void st_rows_kernel(const float* __restrict__ x, int ldx, int rows, int D, int pitch, int normalize,
                                                      bf16* __restrict__ out) {
  const int r = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (r >= rows) return;                                       // wave-uniform
  const float* xr = x + (size_t)r * ldx;
  float inv = 1.f;
  if (normalize) {
    float ss = 0.f;
    for (int c = lane; c < D; c += 64) ss = fmaf(xr[c], xr[c], ss);
    inv = 1.f / fmaxf(sqrtf(wave_sum(ss)), 1e-12f);
  }
  bf16* o = out + (size_t)r * pitch;
  for (int c = lane; c < pitch; c += 64) {
    float v = 0.f;
    if (c < D) v = normalize ? xr[c] * inv : xr[c];
    o[c] = f2bf(v);
  }
}

// ------------------------------------------------------------------------------------------------ 2. scan + selection
// Workgroup (x, y): queries [QT x, + QT), candidate tiles [y tps, y tps + tps).  LDS: Qs [QT][ST_LD] | Cs [ST_CT][ST_LD] | the QT lists,
// k keys each.  part[(b * n_splits + y) * k + l]: the list of query b over this split.
// KEEP IN STEP with sg_scan_kernel (simtopk_groups.hip), which is this body over a group's ranges: a change to the stages, the k loop or
// the selection is made in both, or the two entry points stop giving a pair the same bits.
template <int NQ>
__global__ __launch_bounds__(256) void st_scan_kernel(const bf16* __restrict__ q, const bf16* __restrict__ cand, const int64_t* __restrict__ skip,
                                                      int B, int pitch, int n_cand, int tiles_per_split, int k, tk_key* __restrict__ part) {
  constexpr int QT = 128 * NQ;
  extern __shared__ __align__(16) unsigned char st_smem[];
  bf16* Qs = reinterpret_cast<bf16*>(st_smem);
  bf16* Cs = Qs + QT * ST_LD;
  tk_key* L = reinterpret_cast<tk_key*>(Cs + ST_CT * ST_LD);
  const int tid = threadIdx.x, lane = tid & 63, r = lane & 31, h = lane >> 5;
  const int wq = __builtin_amdgcn_readfirstlane(tid >> 6) * 32 * NQ;      // the wave's first query of the tile
  const int q0 = blockIdx.x * QT;
  const int n_tiles = (n_cand + ST_CT - 1) / ST_CT;
  const int ct_lo = blockIdx.y * tiles_per_split, ct_hi = min(n_tiles, ct_lo + tiles_per_split);
  const int KT = pitch / ST_BK;
  for (int i = tid; i < QT * k; i += 256) L[i] = TK_EMPTY;
  // the query of this lane in each of the wave's NQ query blocks: alive, its skipped candidate, the score of its k-th best (NaN while
  // the list is not full: nothing is below it)
  bool live[NQ];
  int skip_id[NQ];
  float thr[NQ];
#pragma unroll
  for (int nq = 0; nq < NQ; ++nq) {
    const int b = q0 + wq + nq * 32 + r;
    live[nq] = b < B;
    const int64_t sk = (live[nq] && skip) ? skip[b] : -1;
    skip_id[nq] = (sk >= 0 && sk < n_cand) ? (int)sk : -1;
    thr[nq] = st_score(~0u);
  }
  u32x4 gq[4 * NQ], gc[4];
  if (ct_lo < ct_hi) {
    st_load(gq, q, q0, B, pitch, 0);
    st_load(gc, cand, ct_lo * ST_CT, n_cand, pitch, 0);
  }
  for (int ct = ct_lo; ct < ct_hi; ++ct) {
    const int c0 = ct * ST_CT;
    f32x16 acc[NQ][4];
#pragma unroll
    for (int nq = 0; nq < NQ; ++nq)
#pragma unroll
      for (int cb = 0; cb < 4; ++cb)
#pragma unroll
        for (int i = 0; i < 16; ++i) acc[nq][cb][i] = 0.f;
    for (int kt = 0; kt < KT; ++kt) {
      __syncthreads();                                         // the previous stage's reads are done (and the lists are set up)
      st_store(gq, Qs);
      st_store(gc, Cs);
      __syncthreads();
      // the next stage's rows travel while this one is multiplied
      if (kt + 1 < KT) {
        st_load(gq, q, q0, B, pitch, (kt + 1) * ST_BK);
        st_load(gc, cand, c0, n_cand, pitch, (kt + 1) * ST_BK);
      } else if (ct + 1 < ct_hi) {
        st_load(gq, q, q0, B, pitch, 0);
        st_load(gc, cand, c0 + ST_CT, n_cand, pitch, 0);
      }
#pragma unroll
      for (int ks = 0; ks < ST_BK / 16; ++ks) {
        bf16x8 fq[NQ], fc[4];
#pragma unroll
        for (int nq = 0; nq < NQ; ++nq) fq[nq] = *reinterpret_cast<const bf16x8*>(Qs + (wq + nq * 32 + r) * ST_LD + ks * 16 + 8 * h);
#pragma unroll
        for (int cb = 0; cb < 4; ++cb) fc[cb] = *reinterpret_cast<const bf16x8*>(Cs + (cb * 32 + r) * ST_LD + ks * 16 + 8 * h);
#pragma unroll
        for (int nq = 0; nq < NQ; ++nq)
#pragma unroll
          for (int cb = 0; cb < 4; ++cb) acc[nq][cb] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fc[cb], fq[nq], acc[nq][cb], 0, 0, 0);
      }
    }
    // selection.  acc[nq][cb][i]: query wq + 32 nq + r, candidate c0 + 32 cb + (i & 3) + 8 (i >> 2) + 4 h.  The lists of this wave's
    // queries are touched by this wave only; the whole wave walks every step together.
#pragma unroll
    for (int nq = 0; nq < NQ; ++nq) {
      const int cmax = live[nq] ? n_cand - c0 - 4 * h : 0;     // offsets below it are candidates of a live query
      const int skl = skip_id[nq] - c0 - 4 * h;                // the offset that is skipped (none: out of range)
#pragma unroll
      for (int cb = 0; cb < 4; ++cb)
#pragma unroll
        for (int i = 0; i < 16; ++i) {
          const int off = cb * 32 + (i & 3) + 8 * (i >> 2);
          const float s = acc[nq][cb][i];
          const bool pass = off < cmax && off != skl && !(s < thr[nq]);
          unsigned long long bal = __ballot(pass);
          if (!bal) continue;                                  // wave-uniform
          const tk_key mine = ((tk_key)st_order(s) << 32) | (uint32_t)(c0 + 4 * h + off);
          do {
            const int leader = __builtin_amdgcn_readfirstlane(__ffsll(bal) - 1);
            bal &= bal - 1;
            const tk_key key = tk_lane(mine, leader);
            const int lq = wq + nq * 32 + (leader & 31);
            tk_key e = lane < k ? L[lq * k + lane] : TK_EMPTY;
            int pos;
            if (!tk_insert(e, key, k, lane, pos)) continue;
            if (lane >= pos && lane < k) L[lq * k + lane] = e;
            const float kth = st_score((uint32_t)(tk_lane(e, k - 1) >> 32));
            if (r == (leader & 31)) thr[nq] = kth;
          } while (bal);
        }
    }
  }
  __syncthreads();
  for (int i = tid; i < QT * k; i += 256) {
    const int row = i / k, l = i - row * k, b = q0 + row;
    if (b < B) part[((size_t)b * gridDim.y + blockIdx.y) * k + l] = L[i];
  }
}

// ------------------------------------------------------------------------------------------------ 3. merge of the splits
__global__ __launch_bounds__(256) void st_merge_kernel(const tk_key* __restrict__ part, int B, int k, int n_splits, int64_t* __restrict__ idx,
                                                       float* __restrict__ score) {
  const int b = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (b >= B) return;                                          // wave-uniform
  const tk_key cur = tk_merge(part, b, k, n_splits, lane);
  if (lane < k) {
    const bool used = cur != TK_EMPTY;
    idx[(size_t)b * k + lane] = used ? (int64_t)(uint32_t)cur : -1;
    score[(size_t)b * k + lane] = used ? st_score((uint32_t)(cur >> 32)) : -__builtin_inff();
  }
}

// the largest split count a call may use
int st_split_cap(int B, int n_cand, int k, int max_splits) {
  const int q_tiles = (B + st_qt(k) - 1) / st_qt(k), n_tiles = (n_cand + ST_CT - 1) / ST_CT;
  int splits = (ST_TARGET_WGS + q_tiles - 1) / q_tiles;
  if (max_splits > 0 && max_splits < splits) splits = max_splits;
  return splits > n_tiles ? n_tiles : splits;
}
size_t st_ws_bytes(int B, int n_cand, int k, int max_splits) {
  if (B == 0 || n_cand == 0) return 0;
  return ((size_t)B * st_split_cap(B, n_cand, k, max_splits) * k * sizeof(tk_key) + 255) / 256 * 256;
}
bool st_shape_ok(int B, int D, int n_cand, int k, int max_splits) {
  return B >= 0 && D >= 1 && D <= (1 << 20) && n_cand >= 0 && k >= 1 && k <= IA_SIM_TOPK_MAX_K && max_splits >= 0;
}

template <int NQ>
int st_launch_scan(const bf16* q, const bf16* cand, const int64_t* skip, int B, int pitch, int n_cand, int tps, int splits, int k, tk_key* part,
                   hipStream_t stream) {
  constexpr int QT = 128 * NQ;
  const size_t lds = (size_t)(QT + ST_CT) * ST_LD * sizeof(bf16) + (size_t)QT * k * sizeof(tk_key);   // <= 118 KiB; past 64 KiB is asked for
  if (hipFuncSetAttribute((const void*)st_scan_kernel<NQ>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess) return IA_ERR_LAUNCH;
  hipLaunchKernelGGL(st_scan_kernel<NQ>, dim3((B + QT - 1) / QT, splits), dim3(256), lds, stream, q, cand, skip, B, pitch, n_cand, tps, k, part);
  return IA_OK;
}

}  // namespace

extern "C" size_t ia_sim_row_pitch(int D) { return D < 1 ? 0 : (size_t)st_pitch(D); }

extern "C" int ia_sim_rows_bf16(const float* x, int ldx, int rows, int D, int normalize, void* out, hipStream_t stream) {
  if (!x || !out || rows < 0 || D < 1 || D > (1 << 20) || ldx < D || (normalize != 0 && normalize != 1)) return IA_ERR_ARG;
  if (rows == 0) return IA_OK;
  (void)hipGetLastError();
  hipLaunchKernelGGL(st_rows_kernel, dim3((rows + 3) / 4), dim3(256), 0, stream, x, ldx, rows, D, st_pitch(D), normalize, (bf16*)out);
  return ia_check_launch();
}

extern "C" size_t ia_sim_topk_workspace_bytes(int B, int D, int n_cand, int k, int max_splits) {
  if (!st_shape_ok(B, D, n_cand, k, max_splits)) return 0;
  return st_ws_bytes(B, n_cand, k, max_splits);
}

extern "C" int ia_sim_topk(const void* q, const void* cand, int B, int D, int n_cand, const int64_t* skip, int k, int max_splits, int64_t* idx,
                           float* score, void* workspace, size_t workspace_bytes, hipStream_t stream) {
  if (!q || !cand || !idx || !score || !st_shape_ok(B, D, n_cand, k, max_splits)) return IA_ERR_ARG;
  if (((uintptr_t)q | (uintptr_t)cand) & 15) return IA_ERR_ARG;           // rows are read 16 bytes at a time
  const size_t need = st_ws_bytes(B, n_cand, k, max_splits);
  if (need && (!workspace || workspace_bytes < need)) return IA_ERR_ARG;
  if (B == 0) return IA_OK;
  (void)hipGetLastError();
  tk_key* part = reinterpret_cast<tk_key*>(workspace);
  int splits = 0;
  if (n_cand > 0) {
    const int n_tiles = (n_cand + ST_CT - 1) / ST_CT;
    splits = st_split_cap(B, n_cand, k, max_splits);
    const int tps = (n_tiles + splits - 1) / splits;
    splits = (n_tiles + tps - 1) / tps;
    const int pitch = st_pitch(D);
    const int rc = k <= ST_NQ_MAX_K ? st_launch_scan<2>((const bf16*)q, (const bf16*)cand, skip, B, pitch, n_cand, tps, splits, k, part, stream)
                                    : st_launch_scan<1>((const bf16*)q, (const bf16*)cand, skip, B, pitch, n_cand, tps, splits, k, part, stream);
    if (rc != IA_OK) return rc;
  }
  hipLaunchKernelGGL(st_merge_kernel, dim3((B + 3) / 4), dim3(256), 0, stream, part, B, k, splits, idx, score);   // no split: every slot unused
  return ia_check_launch();
}
