// The pair arithmetic and the tile shape shared by the link-prediction rank scan (kglinkpred.hip) and the streaming top-k scan
// (kgtopk.hip): both compute d(q, c) with one fp32 accumulator per pair, summed in k order through lp_step, so the two files produce
// the same bits for the same pair.
#pragma once
#include "common.h"

namespace {

constexpr int LP_QT = 128;   // queries of a workgroup tile
constexpr int LP_CT = 128;   // candidates of a tile
constexpr int LP_DK = 16;    // k depth of one LDS stage
constexpr int LP_LD = LP_QT + 4;
constexpr int LP_TARGET_WGS = 2048;
constexpr int LP_MAX_GRID_Y = 65535;

// the whole arithmetic of a pair step; T = float (listed mode) or f32x2 (two pairs of the scan in one packed instruction)
template <int NORM, typename T>
IA_DEV T lp_step(T acc, T q, T c) {
  const T x = q - c;
  if constexpr (NORM == 2) return __builtin_elementwise_fma(x, x, acc);
  else return acc + __builtin_elementwise_abs(x);
}

// listed-candidates mode: d of one pair, k in order
template <int NORM>
IA_DEV float lp_dist(const float* __restrict__ q, const float* __restrict__ c, int D) {
  float acc = 0.f;
  for (int k = 0; k < D; k += 4) {
    const f32x4 a = *reinterpret_cast<const f32x4*>(q + k), b = *reinterpret_cast<const f32x4*>(c + k);
#pragma unroll
    for (int i = 0; i < 4; ++i) acc = lp_step<NORM>(acc, a[i], b[i]);
  }
  return acc;
}

}  // namespace
