// What the two similarity scans share (simtopk.hip: one query matrix against one candidate matrix; simtopk_groups.hip: many ragged
// (query range x candidate range) problems in one launch): the tile constants, the score <-> key-word map and the staging of a
// 64-element k stage of rows through registers into LDS.  Both scans keep one mfma_f32_32x32x16_bf16 accumulator per pair that walks
// k in stages of ST_BK from a zero start, so the score of a pair is the same bits in either.
#pragma once
#include "common.h"

namespace {

constexpr int ST_CT = 128;            // candidates of a tile
constexpr int ST_BK = 64;             // k depth of one LDS stage = the unit of the row pitch
constexpr int ST_LD = ST_BK + 8;      // LDS row stride in elements: 144 B, the 16 rows of a ds_read_b128 lane group fall on 16 different slots
constexpr int ST_TARGET_WGS = 512;    // two workgroups a CU
constexpr int ST_NQ_MAX_K = 32;       // largest k served by the 256-query tile

// the high word of a key: smaller = better score.  s + 0 turns -0 into +0 (equal scores, one key word)
IA_DEV uint32_t st_order(float s) {
  const uint32_t u = __float_as_uint(s + 0.f);
  return (u & 0x80000000u) ? u : (~u & 0x7FFFFFFFu);
}
// its inverse; the word of TK_EMPTY gives NaN
IA_DEV float st_score(uint32_t w) { return __uint_as_float((w & 0x80000000u) ? w : (~w & 0x7FFFFFFFu)); }

// rows [row0, row0 + 32 N) of `base`, the k columns [k0, k0 + ST_BK): 16 bytes a thread and step; rows at or past n_rows read as zero
template <int N>
IA_DEV void st_load(u32x4 (&g)[N], const bf16* __restrict__ base, int row0, int n_rows, int pitch, int k0) {
#pragma unroll
  for (int s = 0; s < N; ++s) {
    const int e = threadIdx.x + 256 * s, row = row0 + (e >> 3), kc = e & 7;
    g[s] = row < n_rows ? *reinterpret_cast<const u32x4*>(base + (size_t)row * pitch + k0 + kc * 8) : u32x4{0u, 0u, 0u, 0u};
  }
}
template <int N>
IA_DEV void st_store(const u32x4 (&g)[N], bf16* __restrict__ lds) {
#pragma unroll
  for (int s = 0; s < N; ++s) {
    const int e = threadIdx.x + 256 * s;
    *reinterpret_cast<u32x4*>(lds + (e >> 3) * ST_LD + (e & 7) * 8) = g[s];
  }
}

int st_pitch(int D) { return (D + ST_BK - 1) / ST_BK * ST_BK; }
int st_qt(int k) { return k <= ST_NQ_MAX_K ? 256 : 128; }

}  // namespace
