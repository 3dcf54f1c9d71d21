// The similarity scan of simtopk.hip over many small, ragged problems in one launch: G groups, group g pairing the query rows
// [q_off[g], q_off[g + 1]) of one prepared bf16 matrix with the candidate rows [c_off[g], c_off[g + 1]) of another.  The hot path of
// an inverted-file index (item_alignment_amd.retrieval.IVFItemIndex): group = list, candidates = the catalogue stored list by list,
// queries = one gathered row per (query, probed list), sorted by list.
//
// The offsets are DEVICE arrays and nothing is read back: the entry points launch and return.
//   1. tiles:  tile_off[g] = the number of query tiles (QT rows: 256 for k <= 32, 128 above) of the groups before g, one workgroup
//   2. scan:   a grid of the upper bound P / QT + G query tiles x S candidate splits.  Workgroup (x, y) finds its group by a binary
//              search of tile_off for x and leaves when x is past the last tile; then it is st_scan_kernel on the rows
//              [q_lo, q_hi) x the y-th S-th of the group's candidate tiles: the same stages, the same accumulator per pair, the same
//              wave-owned lists (a query's 128 scores of a tile sit in one wave, so insertions need no barrier or atomics).
//              Consecutive x walk the same list, so co-resident workgroups share its rows in L2.
//              A key's low word is the REPORTED id, label[c] (c without labels): the lists come out in (score descending, reported
//              id ascending) whatever the storage order.  skip[p] is a POSITION in the candidate matrix.
//   3. merge:  one wave per query row folds the S lists of its splits (every (row, split) list is written, an empty range writes an
//              empty list, so the partial lists need no clearing)
// ia_sim_topk_fold: one wave per original query folds the lists of its probes, given as rows of the [P, k] result, by the same keys.
// ia_sim_centroid_sums: the fp32 sum of each list's rows for k-means, one thread per (list, column) adding in the given order.
#include "common.h"
#include "../../include/itemalign.h"
#include "topk_list.h"
#include "simscan.h"

namespace {

IA_DEV int sg_clamp(int64_t v, int n) { return v < 0 ? 0 : (v > n ? n : (int)v); }
// the rows [lo, hi) of a group inside a matrix of n rows; offsets out of order give an empty range
IA_DEV void sg_range(const int64_t* __restrict__ off, int g, int n, int& lo, int& hi) {
  lo = sg_clamp(off[g], n);
  hi = sg_clamp(off[g + 1], n);
  if (hi < lo) hi = lo;
}

// ------------------------------------------------------------------------------------------------ 1. query tiles per group
__global__ __launch_bounds__(256) void sg_tiles_kernel(const int64_t* __restrict__ q_off, int G, int P, int QT, int* __restrict__ tile_off) {
  __shared__ int chunk[256];
  const int tid = threadIdx.x, per = (G + 255) / 256, g_lo = min(G, tid * per), g_hi = min(G, g_lo + per);
  int sum = 0;
  for (int g = g_lo; g < g_hi; ++g) {
    int lo, hi;
    sg_range(q_off, g, P, lo, hi);
    sum += (hi - lo + QT - 1) / QT;
  }
  chunk[tid] = sum;
  __syncthreads();
  if (tid == 0) {
    int run = 0;
    for (int i = 0; i < 256; ++i) {
      const int v = chunk[i];
      chunk[i] = run;
      run += v;
    }
    tile_off[G] = run;
  }
  __syncthreads();
  int run = chunk[tid];
  for (int g = g_lo; g < g_hi; ++g) {
    int lo, hi;
    sg_range(q_off, g, P, lo, hi);
    tile_off[g] = run;
    run += (hi - lo + QT - 1) / QT;
  }
}

// ------------------------------------------------------------------------------------------------ 2. scan + selection
// LDS: Qs [QT][ST_LD] | Cs [ST_CT][ST_LD] | the QT lists, k keys each.  part[(p * S + y) * k + l]: the list of query row p over split y.
// KEEP IN STEP with st_scan_kernel (simtopk.hip): from the staging of the first stage to the write-out this is that kernel's body with
// (q0, q_hi, c_lo, c_hi) for (q0, B, 0, n_cand) and the label load; the "same score, same bits" contract of the two entry points (and
// tests/test_sim_topk_groups_gpu.py::test_one_group_covering_everything_is_sim_topk) rests on the two k loops being identical.
template <int NQ>
__global__ __launch_bounds__(256) void sg_scan_kernel(const bf16* __restrict__ q, const bf16* __restrict__ cand, const int64_t* __restrict__ q_off,
                                                      const int64_t* __restrict__ c_off, const int* __restrict__ tile_off,
                                                      const int32_t* __restrict__ label32, const int64_t* __restrict__ label64,
                                                      const int64_t* __restrict__ skip, int G, int P, int n_cand, int pitch, int k,
                                                      tk_key* __restrict__ part) {
  constexpr int QT = 128 * NQ;
  const int t = blockIdx.x;
  if (t >= tile_off[G]) return;                                // workgroup-uniform: the grid is an upper bound
  int g = 0;
  for (int hi = G; hi - g > 1;) {                              // tile_off[g] <= t < tile_off[hi]
    const int mid = (g + hi) >> 1;
    if (tile_off[mid] <= t) g = mid; else hi = mid;
  }
  int q_lo, q_hi, c_lo, c_hi;
  sg_range(q_off, g, P, q_lo, q_hi);
  sg_range(c_off, g, n_cand, c_lo, c_hi);
  const int q0 = q_lo + (t - tile_off[g]) * QT;

  extern __shared__ __align__(16) unsigned char sg_smem[];
  bf16* Qs = reinterpret_cast<bf16*>(sg_smem);
  bf16* Cs = Qs + QT * ST_LD;
  tk_key* L = reinterpret_cast<tk_key*>(Cs + ST_CT * ST_LD);
  const int tid = threadIdx.x, lane = tid & 63, r = lane & 31, h = lane >> 5;
  const int wq = __builtin_amdgcn_readfirstlane(tid >> 6) * 32 * NQ;      // the wave's first query of the tile
  const int n_tiles = (c_hi - c_lo + ST_CT - 1) / ST_CT;
  const int tiles_per_split = (n_tiles + (int)gridDim.y - 1) / (int)gridDim.y;
  const int ct_lo = min(n_tiles, (int)blockIdx.y * tiles_per_split), ct_hi = min(n_tiles, ct_lo + tiles_per_split);
  const int KT = pitch / ST_BK;
  for (int i = tid; i < QT * k; i += 256) L[i] = TK_EMPTY;
  bool live[NQ];
  int skip_at[NQ];
  float thr[NQ];
#pragma unroll
  for (int nq = 0; nq < NQ; ++nq) {
    const int p = q0 + wq + nq * 32 + r;
    live[nq] = p < q_hi;
    const int64_t sk = (live[nq] && skip) ? skip[p] : -1;
    skip_at[nq] = (sk >= c_lo && sk < c_hi) ? (int)sk : -1;
    thr[nq] = st_score(~0u);
  }
  u32x4 gq[4 * NQ], gc[4];
  if (ct_lo < ct_hi) {
    st_load(gq, q, q0, q_hi, pitch, 0);
    st_load(gc, cand, c_lo + ct_lo * ST_CT, c_hi, pitch, 0);
  }
  for (int ct = ct_lo; ct < ct_hi; ++ct) {
    const int c0 = c_lo + ct * ST_CT;
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
      if (kt + 1 < KT) {
        st_load(gq, q, q0, q_hi, pitch, (kt + 1) * ST_BK);
        st_load(gc, cand, c0, c_hi, pitch, (kt + 1) * ST_BK);
      } else if (ct + 1 < ct_hi) {
        st_load(gq, q, q0, q_hi, pitch, 0);
        st_load(gc, cand, c0 + ST_CT, c_hi, pitch, 0);
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
    // acc[nq][cb][i]: query q0 + wq + 32 nq + r, candidate row c0 + 32 cb + (i & 3) + 8 (i >> 2) + 4 h
#pragma unroll
    for (int nq = 0; nq < NQ; ++nq) {
      const int cmax = live[nq] ? c_hi - c0 - 4 * h : 0;       // offsets below it are candidates of this group and of a live query
      const int skl = skip_at[nq] - c0 - 4 * h;                // the offset that is skipped (none: negative)
#pragma unroll
      for (int cb = 0; cb < 4; ++cb)
#pragma unroll
        for (int i = 0; i < 16; ++i) {
          const int off = cb * 32 + (i & 3) + 8 * (i >> 2);
          const float s = acc[nq][cb][i];
          const bool pass = off < cmax && off != skl && !(s < thr[nq]);
          unsigned long long bal = __ballot(pass);
          if (!bal) continue;                                  // wave-uniform
          const int c = c0 + 4 * h + off;
          uint32_t id = (uint32_t)c;
          if (pass && label64) id = (uint32_t)label64[c];
          if (pass && label32) id = (uint32_t)label32[c];
          const tk_key mine = ((tk_key)st_order(s) << 32) | id;
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
    const int row = i / k, l = i - row * k, p = q0 + row;
    if (p < q_hi) part[((size_t)p * gridDim.y + blockIdx.y) * k + l] = L[i];
  }
}

// ------------------------------------------------------------------------------------------------ 3. merge of the splits
IA_DEV void sg_write(tk_key cur, size_t at, int64_t* __restrict__ idx, float* __restrict__ score) {
  const bool used = cur != TK_EMPTY;
  idx[at] = used ? (int64_t)(uint32_t)cur : -1;
  score[at] = used ? st_score((uint32_t)(cur >> 32)) : -__builtin_inff();
}

__global__ __launch_bounds__(256) void sg_merge_kernel(const tk_key* __restrict__ part, const int64_t* __restrict__ q_off, int G, int P, int k,
                                                       int n_splits, int64_t* __restrict__ idx, float* __restrict__ score) {
  const int p = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (p < sg_clamp(q_off[0], P) || p >= sg_clamp(q_off[G], P)) return;    // wave-uniform: a row of no group is left alone
  // offsets out of order or overlapping (refused by the contract, not detectable here) can ask for more tiles than the grid has: some
  // (row, split) lists are then never written and this reads what the workspace held -- in bounds, the row's result unspecified
  const tk_key cur = tk_merge(part, p, k, n_splits, lane);
  if (lane < k) sg_write(cur, (size_t)p * k + lane, idx, score);
}

// ------------------------------------------------------------------------------------------------ fold of a query's probes
__global__ __launch_bounds__(256) void sg_fold_kernel(const int64_t* __restrict__ idx_in, const float* __restrict__ score_in, int n_rows,
                                                      const int64_t* __restrict__ rows_of, int B, int nprobe, int k, int64_t* __restrict__ idx,
                                                      float* __restrict__ score) {
  const int b = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (b >= B) return;                                          // wave-uniform
  tk_key cur = TK_EMPTY;
  for (int j = 0; j < nprobe; ++j) {
    const int64_t p = rows_of[(size_t)b * nprobe + j];
    if (p < 0 || p >= n_rows) continue;                        // wave-uniform: no list
    tk_key mine = TK_EMPTY;
    if (lane < k) {
      const int64_t id = idx_in[(size_t)p * k + lane];
      if (id >= 0) mine = ((tk_key)st_order(score_in[(size_t)p * k + lane]) << 32) | (uint32_t)id;
    }
    for (int t = 0; t < k; ++t) {
      const tk_key key = tk_lane(mine, t);
      int pos;
      if (key == TK_EMPTY || !tk_insert(cur, key, k, lane, pos)) break;
    }
  }
  if (lane < k) sg_write(cur, (size_t)b * k + lane, idx, score);
}

// ------------------------------------------------------------------------------------------------ centroid sums
// thread (list, column): the rows order[list_off[list] .. list_off[list + 1]) added one after the other, so a sum has one writer and
// one order of additions
__global__ __launch_bounds__(256) void sg_centroid_sums_kernel(const bf16* __restrict__ rows, int n_rows, int pitch, int D,
                                                               const int64_t* __restrict__ order, int n_order,
                                                               const int64_t* __restrict__ list_off, float* __restrict__ sums,
                                                               int64_t* __restrict__ counts) {
  const int list = blockIdx.x, col = blockIdx.y * 256 + threadIdx.x;
  int lo, hi;
  sg_range(list_off, list, n_order, lo, hi);
  float acc = 0.f;
  int n = 0;
  for (int i = lo; i < hi; ++i) {
    const int64_t row = order[i];
    if (row < 0 || row >= n_rows) continue;
    ++n;
    if (col < D) acc += bf2f(rows[(size_t)row * pitch + col]);
  }
  if (col < D) sums[(size_t)list * D + col] = acc;
  if (col == 0) counts[list] = n;
}

bool sg_shape_ok(int P, int G, int D, int n_cand, int k, int max_splits) {
  return P >= 0 && G >= 0 && D >= 1 && D <= (1 << 20) && n_cand >= 0 && k >= 1 && k <= IA_SIM_TOPK_MAX_K && max_splits >= 0;
}
// the query tiles a call can have, and the candidate splits it uses: one while the tiles alone fill the chip
int sg_splits(int P, int G, int n_cand, int k, int max_splits) {
  const int tiles = P / st_qt(k) + G, n_tiles = (n_cand + ST_CT - 1) / ST_CT;
  int splits = tiles > 0 ? (ST_TARGET_WGS + tiles - 1) / tiles : 1;
  if (max_splits > 0 && max_splits < splits) splits = max_splits;
  if (splits > n_tiles) splits = n_tiles;
  return splits < 1 ? 1 : splits;
}
size_t sg_table_bytes(int G) { return ((size_t)(G + 1) * sizeof(int) + 255) / 256 * 256; }
size_t sg_ws_bytes(int P, int G, int n_cand, int k, int max_splits) {
  if (P == 0 || G == 0) return 0;
  return sg_table_bytes(G) + ((size_t)P * sg_splits(P, G, n_cand, k, max_splits) * k * sizeof(tk_key) + 255) / 256 * 256;
}

template <int NQ>
int sg_launch_scan(const bf16* q, const bf16* cand, const int64_t* q_off, const int64_t* c_off, const int* tile_off, const void* label,
                   int label_bits, const int64_t* skip, int G, int P, int n_cand, int pitch, int k, int splits, tk_key* part, hipStream_t stream) {
  constexpr int QT = 128 * NQ;
  const size_t lds = (size_t)(QT + ST_CT) * ST_LD * sizeof(bf16) + (size_t)QT * k * sizeof(tk_key);   // <= 118 KiB; past 64 KiB is asked for
  if (hipFuncSetAttribute((const void*)sg_scan_kernel<NQ>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess) return IA_ERR_LAUNCH;
  hipLaunchKernelGGL(sg_scan_kernel<NQ>, dim3(P / QT + G, splits), dim3(256), lds, stream, q, cand, q_off, c_off, tile_off,
                     label_bits == 32 ? (const int32_t*)label : nullptr, label_bits == 64 ? (const int64_t*)label : nullptr, skip, G, P, n_cand,
                     pitch, k, part);
  return IA_OK;
}

}  // namespace

extern "C" size_t ia_sim_topk_groups_workspace_bytes(int P, int G, int D, int n_cand, int k, int max_splits) {
  if (!sg_shape_ok(P, G, D, n_cand, k, max_splits)) return 0;
  return sg_ws_bytes(P, G, n_cand, k, max_splits);
}

extern "C" int ia_sim_topk_groups(const void* q, const void* cand, const int64_t* q_off, const int64_t* c_off, int G, int P, int D, int n_cand,
                                  const void* label, int label_bits, const int64_t* skip, int k, int max_splits, int64_t* idx, float* score,
                                  void* workspace, size_t workspace_bytes, hipStream_t stream) {
  if (!q || !cand || !q_off || !c_off || !idx || !score || !sg_shape_ok(P, G, D, n_cand, k, max_splits)) return IA_ERR_ARG;
  if (label ? (label_bits != 32 && label_bits != 64) : label_bits != 0) return IA_ERR_ARG;
  if (((uintptr_t)q | (uintptr_t)cand) & 15) return IA_ERR_ARG;           // rows are read 16 bytes at a time
  if (((uintptr_t)q_off | (uintptr_t)c_off | (uintptr_t)skip | (uintptr_t)idx) & 7) return IA_ERR_ARG;
  if (((uintptr_t)label & (label_bits == 64 ? 7 : 3)) | ((uintptr_t)score & 3) | ((uintptr_t)workspace & 15)) return IA_ERR_ARG;
  const size_t need = sg_ws_bytes(P, G, n_cand, k, max_splits);
  if (need && (!workspace || workspace_bytes < need)) return IA_ERR_ARG;
  if (P == 0 || G == 0) return IA_OK;
  (void)hipGetLastError();
  int* tile_off = reinterpret_cast<int*>(workspace);
  tk_key* part = reinterpret_cast<tk_key*>((unsigned char*)workspace + sg_table_bytes(G));
  const int splits = sg_splits(P, G, n_cand, k, max_splits), pitch = st_pitch(D);
  hipLaunchKernelGGL(sg_tiles_kernel, dim3(1), dim3(256), 0, stream, q_off, G, P, st_qt(k), tile_off);
  const int rc = k <= ST_NQ_MAX_K ? sg_launch_scan<2>((const bf16*)q, (const bf16*)cand, q_off, c_off, tile_off, label, label_bits, skip, G, P,
                                                      n_cand, pitch, k, splits, part, stream)
                                  : sg_launch_scan<1>((const bf16*)q, (const bf16*)cand, q_off, c_off, tile_off, label, label_bits, skip, G, P,
                                                      n_cand, pitch, k, splits, part, stream);
  if (rc != IA_OK) return rc;
  hipLaunchKernelGGL(sg_merge_kernel, dim3((P + 3) / 4), dim3(256), 0, stream, part, q_off, G, P, k, splits, idx, score);
  return ia_check_launch();
}

extern "C" int ia_sim_topk_fold(const int64_t* idx_in, const float* score_in, int n_rows, const int64_t* rows_of, int B, int nprobe, int k,
                                int64_t* idx, float* score, hipStream_t stream) {
  if (!idx_in || !score_in || !rows_of || !idx || !score || n_rows < 0 || B < 0 || nprobe < 1 || k < 1 || k > IA_SIM_TOPK_MAX_K) return IA_ERR_ARG;
  if ((((uintptr_t)idx_in | (uintptr_t)rows_of | (uintptr_t)idx) & 7) | (((uintptr_t)score_in | (uintptr_t)score) & 3)) return IA_ERR_ARG;
  if (B == 0) return IA_OK;
  (void)hipGetLastError();
  hipLaunchKernelGGL(sg_fold_kernel, dim3((B + 3) / 4), dim3(256), 0, stream, idx_in, score_in, n_rows, rows_of, B, nprobe, k, idx, score);
  return ia_check_launch();
}

extern "C" int ia_sim_centroid_sums(const void* rows, int n_rows, int D, const int64_t* order, int n_order, const int64_t* list_off, int nlist,
                                    float* sums, int64_t* counts, hipStream_t stream) {
  if (!rows || !order || !list_off || !sums || !counts || n_rows < 0 || n_order < 0 || nlist < 0 || D < 1 || D > (1 << 20)) return IA_ERR_ARG;
  if ((((uintptr_t)order | (uintptr_t)list_off | (uintptr_t)counts) & 7) | ((uintptr_t)sums & 3) | ((uintptr_t)rows & 1)) return IA_ERR_ARG;
  if (nlist == 0) return IA_OK;
  (void)hipGetLastError();
  hipLaunchKernelGGL(sg_centroid_sums_kernel, dim3(nlist, (D + 255) / 256), dim3(256), 0, stream, (const bf16*)rows, n_rows, st_pitch(D), D, order,
                     n_order, list_off, sums, counts);
  return ia_check_launch();
}
