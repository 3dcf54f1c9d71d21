// TextCNN tower of the TextCNN two-tower model (reference src/models/text.py:1496-1527: two embedding channels -> Conv2d(2, F, (K, H))
// per filter size K -> relu -> max over time -> concat -> dropout; the two-tower head adds its own dropout, base.py:104-105).
//
// The convolution is not run as a convolution.  With x_c [M = B L, H] the LayerNorm output of channel c and W_s [F, 2, K_s, H] the
// weight of filter size s,
//     pre[b, s, f, t] = bias_s[f] + sum_c sum_{k < K_s} W_s[f, c, k, :] . x_c[b, t + k, :]
// is a shifted sum over the columns of ONE product per channel, the tap projection
//     P [M, NT] (fp32) = x_0 Wtap_0^T + x_1 Wtap_1^T,        Wtap_c [NT, H] (bf16),  NT = F * sum_s K_s,
// column (s, k, f) = F * (K_0 + .. + K_{s-1}) + k * F + f holding W_s[f, c, k, :].  Two ia_gemm_bf16 calls (the second with
// accumulate) write P; no [B, L, K H] patch matrix exists.  The leading dimension of P and the row count of Wtap_c are NT rounded up
// to a multiple of 8 (ia_gemm_bf16 wants N % 4 == 0); the padding rows of Wtap_c are zero.
//
//   ia_textcnn_pack_taps    fp32 conv weights -> the bf16 tap shadow [2][NTP, H]
//   ia_textcnn_pool_fwd     P, biases -> feat [B, NF] fp32 (relu, max over t, both dropouts), argmax [B, NF] int32;  NF = F * S
//   ia_textcnn_pool_bwd_w   dW_s[f, c, k, :] = sum_b g'[b, j] x_c[b, argmax + k, :],  db_s[f] = sum_b g'[b, j]
//   ia_textcnn_pool_bwd_x   dx_0[b, argmax + k, :] += g'[b, j] W_s[f, 0, k, :]   (bf16, every row written)
// g'[b, j] = g[b, j] * (both dropout keeps) / ((1 - p1)(1 - p2)) where argmax >= 0, else 0: because of the max over time every feature
// sends its gradient to one window, so the backward is a gather (dW) and a sparse row scatter (dx) -- no GEMM.
//
// Ties go to the lowest t (F.max_pool1d on the CPU does the same); a feature whose best pre-activation is <= 0 is exactly 0 with
// argmax -1 and sends no gradient (relu' = 0).  No float atomics: dW sums b in index order in one thread per element, dx has one
// writer per row which adds its (s, f) contributions in index order in fp32 and rounds to bf16 once.  Bit-identical from run to run.
#include "common.h"
#include "../../include/itemalign.h"

namespace {

constexpr int MAXS = IA_TEXTCNN_MAX_SIZES;

struct TcShape {
  int S, F, NF, NT, maxK;
  int K[MAXS], off[MAXS];      // off[s] = first column of size s in P
};
struct TcPtrs { const float* p[MAXS]; };
struct TcOut { float* p[MAXS]; };
struct TcDrop { uint32_t thr1, thr2, seed, sid1, sid2; float scale; };

// fills sh from the host array of filter sizes; false = refuse
bool tc_shape(const int* sizes, int S, int F, TcShape& sh) {
  if (!sizes || S <= 0 || S > MAXS || F <= 0) return false;
  sh.S = S; sh.F = F; sh.NF = S * F; sh.maxK = 0;
  long nt = 0;
  for (int s = 0; s < S; ++s) {
    if (sizes[s] <= 0) return false;
    sh.K[s] = sizes[s]; sh.off[s] = (int)nt;
    nt += (long)F * sizes[s];
    if (sizes[s] > sh.maxK) sh.maxK = sizes[s];
    if (nt > (1 << 24)) return false;
  }
  for (int s = S; s < MAXS; ++s) { sh.K[s] = 0; sh.off[s] = 0; }
  sh.NT = (int)nt;
  return true;
}

bool tc_drop(float p1, float p2, uint32_t seed, uint32_t sid1, uint32_t sid2, TcDrop& d) {
  if (!(p1 >= 0.f) || !(p2 >= 0.f) || p1 >= 1.f || p2 >= 1.f) return false;
  d.thr1 = p1 > 0.f ? (uint32_t)(p1 * 65536.f + 0.5f) : 0u;
  d.thr2 = p2 > 0.f ? (uint32_t)(p2 * 65536.f + 0.5f) : 0u;
  if (d.thr1 >= 65536u || d.thr2 >= 65536u) return false;
  const float i1 = d.thr1 ? 1.f / (1.f - (float)d.thr1 / 65536.f) : 1.f, i2 = d.thr2 ? 1.f / (1.f - (float)d.thr2 / 65536.f) : 1.f;
  d.scale = i1 * i2;
  d.seed = seed; d.sid1 = sid1; d.sid2 = sid2;
  return true;
}

// multiplier of feature element e = b * NF + j: 0 if either draw drops it, else 1 / ((1 - p1)(1 - p2)); nothing is drawn at p = 0
IA_DEV float tc_keep(const TcDrop& d, uint32_t e) {
  if (d.thr1) {
    const uint32_t r = ia_rng(d.seed, d.sid1, e >> 1);
    if (((e & 1) ? (r >> 16) : (r & 0xFFFFu)) < d.thr1) return 0.f;
  }
  if (d.thr2) {
    const uint32_t r = ia_rng(d.seed, d.sid2, e >> 1);
    if (((e & 1) ? (r >> 16) : (r & 0xFFFFu)) < d.thr2) return 0.f;
  }
  return d.scale;
}

// gradient that feature (b, j) sends to its window: 0 for a dead or dropped feature
IA_DEV float tc_geff(const float* __restrict__ g, const int32_t* __restrict__ arg, const TcDrop& d, size_t e) {
  if (arg[e] < 0) return 0.f;
  const float m = tc_keep(d, (uint32_t)e);
  return m == 0.f ? 0.f : g[e] * m;
}

// ------------------------------------------------------------------------------------------------ tap packing
// taps[c][off + k F + f][h] = bf16(W[f][c][k][h]); one thread per 8 h
__global__ __launch_bounds__(256) void tc_pack_kernel(const float* __restrict__ W, bf16* __restrict__ taps, int F, int K, int H, int off,
                                                      int NTP) {
  const int H8 = H >> 3;
  const size_t total = (size_t)2 * K * F * H8;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
    const int h8 = (int)(i % H8);
    size_t r = i / H8;
    const int f = (int)(r % F); r /= F;
    const int k = (int)(r % K);
    const int c = (int)(r / K);
    const float* src = W + (((size_t)f * 2 + c) * K + k) * H + (size_t)h8 * 8;
    const f32x4 a = *reinterpret_cast<const f32x4*>(src), b = *reinterpret_cast<const f32x4*>(src + 4);
    bf16x8 o;
#pragma unroll
    for (int q = 0; q < 4; ++q) { o[q] = f2bf(a[q]); o[4 + q] = f2bf(b[q]); }
    *reinterpret_cast<bf16x8*>(taps + ((size_t)c * NTP + off + (size_t)k * F + f) * H + (size_t)h8 * 8) = o;
  }
}

// the padding rows NT .. NTP-1 of both channels
__global__ __launch_bounds__(256) void tc_pack_pad_kernel(bf16* __restrict__ taps, int NT, int NTP, int H) {
  const size_t per = (size_t)(NTP - NT) * H, total = 2 * per;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
    const size_t c = i / per, r = i % per;
    taps[(c * NTP + NT) * H + r] = f2bf(0.f);
  }
}

// ------------------------------------------------------------------------------------------------ pool forward
// Workgroup = (32 features j, 8 slices of t) of one b.  Lane x owns feature j0 + x: for a fixed (t, k) the 32 lanes read consecutive
// columns of one row of P (runs of F columns per filter size), the two half-waves the rows t and t + 1.  Slice y walks t = y, y + 8, ..:
// pre = ((P[t][k=0] + P[t+1][k=1]) + ..) + bias, K roundings; a strict > keeps the lowest t of the slice, the slices are joined through
// LDS with ties to the lower t.  Every element of P is read exactly once.
constexpr int TC_FX = 32, TC_TY = 8;

__global__ __launch_bounds__(TC_FX * TC_TY) void tc_pool_fwd_kernel(const float* __restrict__ P, int ldp, TcPtrs bias, TcShape sh, int B,
                                                                    int L, TcDrop d, float* __restrict__ feat,
                                                                    int32_t* __restrict__ argmax) {
  __shared__ float s_best[TC_TY][TC_FX];
  __shared__ int s_arg[TC_TY][TC_FX];
  const int x = threadIdx.x, y = threadIdx.y, b = blockIdx.y;
  const int j = blockIdx.x * TC_FX + x;
  const bool live = j < sh.NF;
  float best = -INFINITY;
  int arg = -1;
  if (live) {
    const int s = j / sh.F, f = j - s * sh.F, K = sh.K[s];
    const float bs = bias.p[s][f];
    const float* col = P + (size_t)b * L * ldp + sh.off[s] + f;
    for (int t = y; t + K <= L; t += TC_TY) {
      const float* p = col + (size_t)t * ldp;
      float acc = p[0];
      for (int k = 1; k < K; ++k) acc += p[(size_t)k * ldp + (size_t)k * sh.F];
      acc += bs;
      if (acc > best) { best = acc; arg = t; }
    }
  }
  s_best[y][x] = best; s_arg[y][x] = arg;
  __syncthreads();
  if (y == 0 && live) {
    for (int q = 1; q < TC_TY; ++q) {
      const float v = s_best[q][x];
      const int a = s_arg[q][x];
      if (a >= 0 && (v > best || (v == best && a < arg))) { best = v; arg = a; }
    }
    const size_t e = (size_t)b * sh.NF + j;
    if (!(best > 0.f)) { feat[e] = 0.f; argmax[e] = -1; }
    else { feat[e] = best * tc_keep(d, (uint32_t)e); argmax[e] = arg; }
  }
}

// ------------------------------------------------------------------------------------------------ weight gradient
// Workgroup (column n = (s, k, f) of P, channel c): thread owns 8 h at a time and adds b = 0 .. B-1 in order, one fma each.
// db_s[f] comes from the (k = 0, c = 0) workgroup's first thread.
__global__ __launch_bounds__(128) void tc_bwd_w_kernel(const float* __restrict__ g, const int32_t* __restrict__ arg,
                                                       const bf16* __restrict__ x0, const bf16* __restrict__ x1, TcShape sh, int B, int L,
                                                       int H, TcDrop d, TcOut dW, TcOut db) {
  const int n = blockIdx.x, c = blockIdx.y;
  int s = 0;
  while (s + 1 < sh.S && n >= sh.off[s + 1]) ++s;
  const int K = sh.K[s], k = (n - sh.off[s]) / sh.F, f = (n - sh.off[s]) - k * sh.F, j = s * sh.F + f;
  const bf16* __restrict__ x = c ? x1 : x0;
  float* out = dW.p[s] + (((size_t)f * 2 + c) * K + k) * H;
  for (int h = threadIdx.x * 8; h < H; h += 128 * 8) {
    float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    for (int b = 0; b < B; ++b) {
      const size_t e = (size_t)b * sh.NF + j;
      const float ge = tc_geff(g, arg, d, e);
      const int a = arg[e];
      if (ge == 0.f || a + K > L) continue;          // (an argmax the forward cannot have written reads nothing)
      const bf16x8 v = *reinterpret_cast<const bf16x8*>(x + ((size_t)b * L + a + k) * H + h);
#pragma unroll
      for (int q = 0; q < 8; ++q) acc[q] = fmaf(ge, bf2f(v[q]), acc[q]);
    }
    *reinterpret_cast<f32x4*>(out + h) = f32x4{acc[0], acc[1], acc[2], acc[3]};
    *reinterpret_cast<f32x4*>(out + h + 4) = f32x4{acc[4], acc[5], acc[6], acc[7]};
  }
  if (k == 0 && c == 0 && threadIdx.x == 0 && db.p[s]) {
    float sum = 0.f;
    for (int b = 0; b < B; ++b) sum += tc_geff(g, arg, d, (size_t)b * sh.NF + j);
    db.p[s][f] = sum;
  }
}

// ------------------------------------------------------------------------------------------------ input gradient (channel 0)
// Workgroup = one row (b, r) of dx.  The g' and argmax of sample b go to LDS in chunks of 256 features; every thread then walks the
// features in (s, f) order -- at most one k = r - argmax of a feature lands on this row -- and adds g' W_s[f, 0, k, h..h+7] in fp32.
__global__ __launch_bounds__(128) void tc_bwd_x_kernel(const float* __restrict__ g, const int32_t* __restrict__ arg, TcPtrs W, TcShape sh,
                                                       int B, int L, int H, TcDrop d, bf16* __restrict__ dx) {
  __shared__ float s_g[256];
  __shared__ int s_k[256];
  const size_t m = blockIdx.x;
  const int b = (int)(m / L), r = (int)(m % L);
  for (int h0 = 0; h0 < H; h0 += 128 * 8) {
    const int h = h0 + threadIdx.x * 8;
    float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    for (int j0 = 0; j0 < sh.NF; j0 += 256) {
      __syncthreads();
      for (int i = threadIdx.x; i < 256; i += 128) {
        const int j = j0 + i;
        float ge = 0.f;
        int k = -1;
        if (j < sh.NF) {
          const size_t e = (size_t)b * sh.NF + j;
          const int a = arg[e];
          const int kk = r - a;
          if (a >= 0 && kk >= 0 && kk < sh.K[j / sh.F]) {
            ge = tc_geff(g, arg, d, e);
            if (ge != 0.f) k = kk;
          }
        }
        s_g[i] = ge; s_k[i] = k;
      }
      __syncthreads();
      if (h < H) {
        const int jn = sh.NF - j0 < 256 ? sh.NF - j0 : 256;
        for (int i = 0; i < jn; ++i) {
          const int k = s_k[i];
          if (k < 0) continue;
          const int j = j0 + i, s = j / sh.F, f = j - s * sh.F;
          const float ge = s_g[i];
          const float* w = W.p[s] + (((size_t)f * 2) * sh.K[s] + k) * H + h;
          const f32x4 a = *reinterpret_cast<const f32x4*>(w), c = *reinterpret_cast<const f32x4*>(w + 4);
#pragma unroll
          for (int q = 0; q < 4; ++q) { acc[q] = fmaf(ge, a[q], acc[q]); acc[4 + q] = fmaf(ge, c[q], acc[4 + q]); }
        }
      }
    }
    if (h < H) {
      bf16x8 o;
#pragma unroll
      for (int q = 0; q < 8; ++q) o[q] = f2bf(acc[q]);
      *reinterpret_cast<bf16x8*>(dx + m * H + h) = o;
    }
  }
}

int tc_grid(size_t items) { size_t gsz = (items + 255) / 256; return (int)(gsz < 4096 ? (gsz ? gsz : 1) : 4096); }

}  // namespace

extern "C" int ia_textcnn_pack_taps(const float* const* W, const int* sizes, int S, int F, int H, void* taps, hipStream_t stream) {
  (void)hipGetLastError();
  TcShape sh;
  if (!W || !taps || H <= 0 || (H & 7) || !tc_shape(sizes, S, F, sh)) return IA_ERR_ARG;
  for (int s = 0; s < S; ++s) if (!W[s] || ((uintptr_t)W[s] & 15)) return IA_ERR_ARG;
  if ((uintptr_t)taps & 15) return IA_ERR_ARG;
  const int NTP = (sh.NT + 7) & ~7;
  for (int s = 0; s < S; ++s) {
    const size_t items = (size_t)2 * sh.K[s] * F * (H >> 3);
    hipLaunchKernelGGL(tc_pack_kernel, dim3(tc_grid(items)), dim3(256), 0, stream, W[s], (bf16*)taps, F, sh.K[s], H, sh.off[s], NTP);
  }
  if (NTP > sh.NT)
    hipLaunchKernelGGL(tc_pack_pad_kernel, dim3(tc_grid((size_t)2 * (NTP - sh.NT) * H)), dim3(256), 0, stream, (bf16*)taps, sh.NT, NTP, H);
  return ia_check_launch();
}

extern "C" int ia_textcnn_pool_fwd(const float* P, int ldp, const float* const* bias, const int* sizes, int S, int F, int B, int L,
                                   float p1, float p2, uint32_t seed, uint32_t stream_id1, uint32_t stream_id2, float* feat,
                                   int32_t* argmax, hipStream_t stream) {
  (void)hipGetLastError();
  TcShape sh;
  TcDrop d;
  if (!P || !bias || !feat || !argmax || B <= 0 || L <= 0 || !tc_shape(sizes, S, F, sh)) return IA_ERR_ARG;
  if (L < sh.maxK || ldp < sh.NT || B > 65535 || (size_t)B * sh.NF >= ((size_t)1 << 32)) return IA_ERR_ARG;
  if (!tc_drop(p1, p2, seed, stream_id1, stream_id2, d)) return IA_ERR_ARG;
  TcPtrs bp;
  for (int s = 0; s < MAXS; ++s) { bp.p[s] = s < S ? bias[s] : nullptr; if (s < S && !bias[s]) return IA_ERR_ARG; }
  hipLaunchKernelGGL(tc_pool_fwd_kernel, dim3((sh.NF + TC_FX - 1) / TC_FX, B), dim3(TC_FX, TC_TY), 0, stream, P, ldp, bp, sh, B, L, d, feat,
                     argmax);
  return ia_check_launch();
}

extern "C" int ia_textcnn_pool_bwd_w(const float* g, const int32_t* argmax, const void* x0, const void* x1, const int* sizes, int S, int F,
                                     int B, int L, int H, float p1, float p2, uint32_t seed, uint32_t stream_id1, uint32_t stream_id2,
                                     float* const* dW, float* const* db, hipStream_t stream) {
  (void)hipGetLastError();
  TcShape sh;
  TcDrop d;
  if (!g || !argmax || !x0 || !x1 || !dW || B <= 0 || L <= 0 || H <= 0 || (H & 7) || !tc_shape(sizes, S, F, sh)) return IA_ERR_ARG;
  if (L < sh.maxK || (size_t)B * sh.NF >= ((size_t)1 << 32)) return IA_ERR_ARG;
  if (((uintptr_t)x0 & 15) || ((uintptr_t)x1 & 15)) return IA_ERR_ARG;
  if (!tc_drop(p1, p2, seed, stream_id1, stream_id2, d)) return IA_ERR_ARG;
  TcOut wp, bp;
  for (int s = 0; s < MAXS; ++s) {
    wp.p[s] = s < S ? dW[s] : nullptr;
    bp.p[s] = (s < S && db) ? db[s] : nullptr;
    if (s < S && (!dW[s] || ((uintptr_t)dW[s] & 15))) return IA_ERR_ARG;
  }
  hipLaunchKernelGGL(tc_bwd_w_kernel, dim3(sh.NT, 2), dim3(128), 0, stream, g, argmax, (const bf16*)x0, (const bf16*)x1, sh, B, L, H, d, wp,
                     bp);
  return ia_check_launch();
}

extern "C" int ia_textcnn_pool_bwd_x(const float* g, const int32_t* argmax, const float* const* W, const int* sizes, int S, int F, int B,
                                     int L, int H, float p1, float p2, uint32_t seed, uint32_t stream_id1, uint32_t stream_id2, void* dx,
                                     hipStream_t stream) {
  (void)hipGetLastError();
  TcShape sh;
  TcDrop d;
  if (!g || !argmax || !W || !dx || B <= 0 || L <= 0 || H <= 0 || (H & 7) || !tc_shape(sizes, S, F, sh)) return IA_ERR_ARG;
  if (L < sh.maxK || (size_t)B * sh.NF >= ((size_t)1 << 32) || (size_t)B * L >= ((size_t)1 << 31) || ((uintptr_t)dx & 15)) return IA_ERR_ARG;
  if (!tc_drop(p1, p2, seed, stream_id1, stream_id2, d)) return IA_ERR_ARG;
  TcPtrs wp;
  for (int s = 0; s < MAXS; ++s) {
    wp.p[s] = s < S ? W[s] : nullptr;
    if (s < S && (!W[s] || ((uintptr_t)W[s] & 15))) return IA_ERR_ARG;
  }
  hipLaunchKernelGGL(tc_bwd_x_kernel, dim3((unsigned)((size_t)B * L)), dim3(128), 0, stream, g, argmax, wp, sh, B, L, H, d, (bf16*)dx);
  return ia_check_launch();
}
