// Knowledge-graph completion on the PKGM / TransE tables (reference torchkge inference.py EntityInference / RelationInference): the k
// best candidates of every query, without a [B, n_cand] score matrix.  The candidate table streams through the 128 x 128 LDS tiles of
// the rank scan (kglinkpred.hip); only per-query lists of k entries are kept.
//
// One ia_kgpt_topk call answers B queries of one mode:
//   TAILS: q = ent[a] + rel[b], candidates = ent rows;  HEADS: q = ent[a] - rel[b], candidates = ent rows;
//   RELS:  q = ent[b] - ent[a], candidates = rel rows
//   d(q, c) as in kgpair.h (one fp32 accumulator per pair, k in order), score = -d
//   1. prep:   q rows into the workspace (one wave per query); ids out of range mark the query dead
//   2. scan:   workgroup (split, query tile) walks its candidate tiles; after each tile a thread tests the 64 distances it holds
//              against the current k-th best of their queries (one compare per pair); a candidate that passes is looked up in the
//              query's filter group (binary search, the groups are sorted) and inserted into the query's sorted list in LDS
//   3. merge:  one wave per query folds the lists of the splits
// A list entry is one 64-bit key (bits of d) << 32 | id.  d >= +0, so the unsigned order of the keys is the total order (d ascending,
// id ascending) = (score descending, id ascending); keys are unique, so the k smallest keys of a candidate set do not depend on the
// order in which the candidates arrive: the result is a function of the tables, the query and the filter alone.
// All candidates of a query within a tile sit in 16 lanes of one wave (kglinkpred.hip's thread map), so a query's list belongs to one
// wave: insertions need no barrier.  An insertion is done by the whole wave, lane l holding entry l.
#include "common.h"
#include "../../include/itemalign.h"
#include "kgpair.h"
#include "topk_list.h"   // tk_key, TK_EMPTY, tk_lane, tk_up1, tk_insert, tk_merge

namespace {

IA_DEV tk_key tk_make(float d, int id) { return ((tk_key)__float_as_uint(d) << 32) | (uint32_t)id; }

// ------------------------------------------------------------------------------------------------ 1. query rows
__global__ __launch_bounds__(256) void tk_prep_kernel(const float* __restrict__ ent, const float* __restrict__ rel, const int64_t* __restrict__ a,
                                                      const int64_t* __restrict__ bb, int B, int D, int n_ent, int n_rel, int mode,
                                                      float* __restrict__ q, int* __restrict__ alive) {
  const int b = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (b >= B) return;                                          // wave-uniform
  const int64_t ia = a[b], ib = bb[b];
  const bool rels = mode == IA_KGPT_TOPK_RELS;
  const bool ok = ia >= 0 && ia < n_ent && ib >= 0 && ib < (rels ? n_ent : n_rel);
  // x (+|-) y: TAILS ent[a] + rel[b], HEADS ent[a] - rel[b], RELS ent[b] - ent[a]
  const float* xr = ent + (ok ? (size_t)(rels ? ib : ia) * D : 0);
  const float* yr = (rels ? ent : rel) + (ok ? (size_t)(rels ? ia : ib) * D : 0);
  float* dst = q + (size_t)b * D;
  for (int c = lane * 4; c < D; c += 256) {
    f32x4 v = {0.f, 0.f, 0.f, 0.f};
    if (ok) {
      const f32x4 x = *reinterpret_cast<const f32x4*>(xr + c), y = *reinterpret_cast<const f32x4*>(yr + c);
      v = mode == IA_KGPT_TOPK_TAILS ? x + y : x - y;
    }
    *reinterpret_cast<f32x4*>(dst + c) = v;
  }
  if (lane == 0) alive[b] = ok ? 1 : 0;
}

// ------------------------------------------------------------------------------------------------ 2. scan + selection
IA_DEV int tk_row(int i) { return (i & 3) + ((i >> 2) << 6); }   // kglinkpred.hip's lp_row: i in [0, 8) -> offset of the i-th owned row

// true when id is a member of the sorted range ids[lo, hi)
IA_DEV bool tk_member(const int64_t* __restrict__ ids, int64_t lo, int64_t hi, int64_t id) {
  while (lo < hi) {
    const int64_t mid = lo + ((hi - lo) >> 1);
    const int64_t v = ids[mid];
    if (v == id) return true;
    if (v < id) lo = mid + 1; else hi = mid;
  }
  return false;
}

// The selection of one owned query row (the same slot i in every lane, so the 16 lanes of a group share the row `qr`): `pend` marks the
// lane's candidates that passed the register test against the row's k-th best.  Whole wave, in step.
IA_DEV void tk_select(const float (&d)[8], unsigned pend, int qr, int b, int cbase, int k, const int64_t* __restrict__ grp_off,
                      const int64_t* __restrict__ grp_ids, int n_grp, const int64_t* __restrict__ q_grp, tk_key* __restrict__ L) {
  const int lane = threadIdx.x & 63;
  // exact test (the register test let equal distances through) and the filter, all lanes at once
  if (pend) {
    const tk_key thr = L[qr * k + k - 1];
    int64_t lo = 0, hi = 0;
    if (grp_off) {
      const int64_t g = q_grp[b];
      if (g >= 0 && g < n_grp) { lo = grp_off[g]; hi = grp_off[g + 1]; }
    }
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      if (!((pend >> j) & 1)) continue;
      const int c = cbase + tk_row(j);
      if (tk_make(d[j], c) >= thr || tk_member(grp_ids, lo, hi, c)) pend &= ~(1u << j);
    }
  }
  // one insertion at a time; after each, the lanes of that row drop what the new k-th best beats
  for (;;) {
    const unsigned long long bal = __ballot(pend != 0);
    if (!bal) break;
    const int leader = __builtin_amdgcn_readfirstlane(__ffsll(bal) - 1);
    const int j = pend ? __ffs(pend) - 1 : 0;
    float dj = d[0];
#pragma unroll
    for (int jj = 1; jj < 8; ++jj) dj = j == jj ? d[jj] : dj;
    const tk_key key = tk_lane(tk_make(dj, cbase + tk_row(j)), leader);
    const int lq = __builtin_amdgcn_readlane(qr, leader);
    if (lane == leader) pend &= pend - 1;
    tk_key e = lane < k ? L[lq * k + lane] : TK_EMPTY;
    int pos;
    if (!tk_insert(e, key, k, lane, pos)) continue;
    if (lane >= pos && lane < k) L[lq * k + lane] = e;
    const float thr = __uint_as_float((uint32_t)(tk_lane(e, k - 1) >> 32));   // NaN while the list is not full: nothing is dropped
    if (qr == lq) {
#pragma unroll
      for (int j2 = 0; j2 < 8; ++j2)
        if (d[j2] > thr) pend &= ~(1u << j2);
    }
  }
}

// Workgroup (x, y): queries [128 (qt0 + y), + 128), candidate tiles [x tps, x tps + tps); thread map and k loop as lp_scan_kernel.
// L: the 128 lists, k keys each (dynamic LDS).  part[(b * n_splits + x) * k + l]: the list of query b over this split.
template <int NORM>
__global__ __launch_bounds__(256) void tk_scan_kernel(const float* __restrict__ cand, const float* __restrict__ q, const int* __restrict__ alive,
                                                      int B, int D, int n_cand, int tiles_per_split, int qt0, int k,
                                                      const int64_t* __restrict__ grp_off, const int64_t* __restrict__ grp_ids, int n_grp,
                                                      const int64_t* __restrict__ q_grp, tk_key* __restrict__ part) {
  __shared__ float Qs[LP_DK][LP_LD];
  __shared__ float Cs[LP_DK][LP_LD];
  extern __shared__ __align__(16) tk_key L[];
  const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
  const int q0 = (qt0 + (int)blockIdx.y) * LP_QT;
  const int n_tiles = (n_cand + LP_CT - 1) / LP_CT;
  const int ct_lo = blockIdx.x * tiles_per_split, ct_hi = min(n_tiles, ct_lo + tiles_per_split);
  for (int i = tid; i < LP_QT * k; i += 256) L[i] = TK_EMPTY;
  unsigned my_alive = 0;
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const int b = q0 + ty * 4 + tk_row(i);
    my_alive |= (b < B && alive[b]) ? 1u << i : 0u;
  }
  __syncthreads();
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
        const int e = tid + 256 * s, row = e >> 2, kk = (e & 3) * 4, kd = k0 + kk;
        const int gq = q0 + row, gc = c0 + row;
        vq[s] = (gq < B && kd < D) ? *reinterpret_cast<const f32x4*>(q + (size_t)gq * D + kd) : f32x4{0.f, 0.f, 0.f, 0.f};
        vc[s] = (gc < n_cand && kd < D) ? *reinterpret_cast<const f32x4*>(cand + (size_t)gc * D + kd) : f32x4{0.f, 0.f, 0.f, 0.f};
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
    // selection: the lists of this wave's 32 queries are touched by this wave only
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const int qr = ty * 4 + tk_row(i);
      const float thr = __uint_as_float((uint32_t)(L[qr * k + k - 1] >> 32));   // d of the k-th best; NaN (TK_EMPTY) while not full
      float d[8];
      unsigned pend = 0;
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        d[j] = acc[i][j >> 1][j & 1];
        const bool pass = c0 + tx * 4 + tk_row(j) < n_cand && !(d[j] > thr);
        pend |= pass ? 1u << j : 0u;
      }
      if (!((my_alive >> i) & 1)) pend = 0;
      if (__ballot(pend != 0)) tk_select(d, pend, qr, q0 + qr, c0 + tx * 4, k, grp_off, grp_ids, n_grp, q_grp, L);
    }
  }
  __syncthreads();
  for (int i = tid; i < LP_QT * k; i += 256) {
    const int row = i / k, l = i - row * k, b = q0 + row;
    if (b < B) part[((size_t)b * gridDim.x + blockIdx.x) * k + l] = L[i];
  }
}

// ------------------------------------------------------------------------------------------------ 3. merge of the splits
// One wave per query: the running list sits one entry per lane; every split's list (sorted) is inserted entry by entry until one fails
// (tk_merge).
__global__ __launch_bounds__(256) void tk_merge_kernel(const tk_key* __restrict__ part, int B, int k, int n_splits, int64_t* __restrict__ idx,
                                                       float* __restrict__ score) {
  const int b = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (b >= B) return;                                          // wave-uniform
  const tk_key cur = tk_merge(part, b, k, n_splits, lane);
  if (lane < k) {
    const bool used = cur != TK_EMPTY;
    idx[(size_t)b * k + lane] = used ? (int64_t)(uint32_t)cur : -1;
    score[(size_t)b * k + lane] = used ? -__uint_as_float((uint32_t)(cur >> 32)) : -__builtin_inff();
  }
}

int tk_split_cap(int B, int max_splits) {
  const int q_tiles = (B + LP_QT - 1) / LP_QT;
  const int splits = (LP_TARGET_WGS + q_tiles - 1) / q_tiles;   // the rank scan's choice before its clamp to the tile count
  return max_splits > 0 && max_splits < splits ? max_splits : splits;
}

struct TkWs {
  float* q;
  int* alive;
  tk_key* part;
  size_t bytes;
};

TkWs tk_ws_layout(char* base, int B, int D, int k, int max_splits) {
  TkWs w{};
  size_t off = 0;
  auto take = [&](size_t bytes) { char* p = base ? base + off : nullptr; off += (bytes + 255) / 256 * 256; return p; };
  w.q = reinterpret_cast<float*>(take((size_t)B * D * 4));
  w.alive = reinterpret_cast<int*>(take((size_t)B * 4));
  w.part = reinterpret_cast<tk_key*>(take((size_t)B * tk_split_cap(B, max_splits) * k * sizeof(tk_key)));
  w.bytes = off;
  return w;
}

}  // namespace

extern "C" size_t ia_kgpt_topk_workspace_bytes(int B, int D, int n_cand, int k, int max_splits) {
  (void)n_cand;                                                 // the size does not depend on the candidate count
  if (B <= 0 || D <= 0 || k < 1 || k > IA_KGPT_TOPK_MAX_K || max_splits < 0) return 0;
  return tk_ws_layout(nullptr, B, D, k, max_splits).bytes;
}

extern "C" int ia_kgpt_topk(const float* ent, const float* rel, const int64_t* a, const int64_t* b, int B, int D, int n_ent, int n_rel, int norm,
                            int mode, const int64_t* grp_off, const int64_t* grp_ids, int n_grp, const int64_t* q_grp, int k, int max_splits,
                            int64_t* idx, float* score, void* workspace, size_t workspace_bytes, hipStream_t stream) {
  if (!ent || !rel || !a || !b || !idx || !score) return IA_ERR_ARG;
  if (B <= 0 || D <= 0 || (D & 3) || n_ent <= 0 || n_rel <= 0 || (norm != 1 && norm != 2)) return IA_ERR_ARG;
  if (mode != IA_KGPT_TOPK_TAILS && mode != IA_KGPT_TOPK_HEADS && mode != IA_KGPT_TOPK_RELS) return IA_ERR_ARG;
  if (k < 1 || k > IA_KGPT_TOPK_MAX_K || max_splits < 0) return IA_ERR_ARG;
  if (grp_off && (!grp_ids || !q_grp || n_grp < 0)) return IA_ERR_ARG;
  const int n_cand = mode == IA_KGPT_TOPK_RELS ? n_rel : n_ent;
  if (!workspace || workspace_bytes < ia_kgpt_topk_workspace_bytes(B, D, n_cand, k, max_splits)) return IA_ERR_WORKSPACE;
  (void)hipGetLastError();
  const TkWs w = tk_ws_layout((char*)workspace, B, D, k, max_splits);
  const float* cand = mode == IA_KGPT_TOPK_RELS ? rel : ent;
  const dim3 blk(256);
  const int n_tiles = (n_cand + LP_CT - 1) / LP_CT, q_tiles = (B + LP_QT - 1) / LP_QT;
  int splits = tk_split_cap(B, max_splits);
  splits = splits > n_tiles ? n_tiles : splits;
  const int tps = (n_tiles + splits - 1) / splits;
  splits = (n_tiles + tps - 1) / tps;
  const size_t lds = (size_t)LP_QT * k * sizeof(tk_key);       // + 16.5 KB static: past 64 KiB from k = 47, asked for explicitly
  const void* scan = norm == 2 ? (const void*)tk_scan_kernel<2> : (const void*)tk_scan_kernel<1>;
  if (hipFuncSetAttribute(scan, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess) return IA_ERR_LAUNCH;
  hipLaunchKernelGGL(tk_prep_kernel, dim3((B + 3) / 4), blk, 0, stream, ent, rel, a, b, B, D, n_ent, n_rel, mode, w.q, w.alive);
  for (int qt0 = 0; qt0 < q_tiles; qt0 += LP_MAX_GRID_Y) {
    const dim3 sgrid(splits, min(LP_MAX_GRID_Y, q_tiles - qt0));
    if (norm == 2)
      hipLaunchKernelGGL(tk_scan_kernel<2>, sgrid, blk, lds, stream, cand, w.q, w.alive, B, D, n_cand, tps, qt0, k, grp_off, grp_ids, n_grp, q_grp,
                         w.part);
    else
      hipLaunchKernelGGL(tk_scan_kernel<1>, sgrid, blk, lds, stream, cand, w.q, w.alive, B, D, n_cand, tps, qt0, k, grp_off, grp_ids, n_grp, q_grp,
                         w.part);
  }
  hipLaunchKernelGGL(tk_merge_kernel, dim3((B + 3) / 4), blk, 0, stream, w.part, B, k, splits, idx, score);
  return ia_check_launch();
}
