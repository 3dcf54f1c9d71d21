// Symmetric contrastive loss between the text and the image embeddings of a batch (CoCaForPretraining's contrastive part; reference
// src/models/multimodal.py:843-933), gfx950.  With s = expf(*log_scale):
//
//   ia_contrastive_fwd : sim[i][j] = s sum_k text[i][k] image[j][k], lse_row[i] = log sum_j exp(sim[i][j]), lse_col[j] = log sum_i
//                        exp(sim[i][j]), loss = 0.5 (mean_i (lse_row[i] - sim[i][i]) + mean_j (lse_col[j] - sim[j][j]))
//   ia_contrastive_bwd : G[i][j] = dloss (0.5 / B) (exp(sim[i][j] - lse_row[i]) + exp(sim[i][j] - lse_col[j]) - 2 [i == j]),
//                        dtext = s G image, dimage = s G^T text, dlog_scale (+)= sum_ij G[i][j] sim[i][j]
//
// At the real shape (B = 64, H = 768) all of it is 3 x 6.3 MFLOP over 0.4 MB of operands (two [B, H] fp32 inputs, two outputs, the
// [B, B] sim and G): launch-sized kernels, plain fp32 FMA on the VALU.  The embeddings are not normalised, so |sim| runs into the
// hundreds and the softmax needs every bit of the fp32 dot: no MFMA, no bf16.  Every sum has a fixed order and there are no atomics:
// two runs agree bit for bit.  expf / logf are the library functions (1 ulp).  The pad columns H .. ld-1 of the inputs and B .. lds-1
// of sim are never read, those of the outputs never written.
//
// fp32 summation chains, as tests/contrastive_reference.py counts them (roundings on the longest path):
//   * a dot product of length n kept in four accumulators (term k goes to accumulator k % 4, fmaf, in k order), combined as
//     (a0 + a1) + (a2 + a3): ceil(n / 4) + 2.  sim has n = H and one more rounding for the product with s; dtext and dimage have
//     n = B and one more for the product with s;
//   * a sum of n terms over one wave (lane l takes terms l, l + 64, ... in order, then wave_sum: 4 butterfly steps + 2):
//     ceil(n / 64) + 6.  The sums of exponentials of lse_row / lse_col, the two means of the loss, a row's part of dlog_scale (fmaf)
//     and the sum of those parts all have n = B;
//   * loss = 0.5 (R / B + C / B): two divisions next to each other and one addition [2], the product with 0.5 is exact;
//   * G: c = dloss * (0.5f / B) [2], (p + q) - 2 [i == j] [2], the product with c [1];
//   * dlog_scale: the sum of the row parts, one more rounding when it accumulates.
#include <limits.h>
#include <math.h>
#include "common.h"

namespace {

constexpr int CT_TILE = 16;        // a workgroup of ia_contrastive_fwd's first kernel owns a 16 x 16 tile of sim
constexpr int CT_KSTEP = 32;       // and walks H in steps of 32 staged through LDS
constexpr int CT_THREADS = 256;

// sim tile (ti, tj): thread (y, x) owns sim[16 ti + y][16 tj + x].  Rows past B and columns past H are staged as zeros (fmaf(0, 0, a) = a
// exactly, so the chain is that of H terms), nothing past them is read.
__global__ __launch_bounds__(CT_THREADS) void contrastive_sim_kernel(const float* __restrict__ text, int ldt, const float* __restrict__ image,
                                                                     int ldi, const float* __restrict__ log_scale, float* __restrict__ sim,
                                                                     int lds, int B, int H, int ntile) {
  __shared__ float ts[CT_TILE][CT_KSTEP + 1], is[CT_TILE][CT_KSTEP + 1];
  const int t = threadIdx.x, y = t >> 4, x = t & 15;
  const int i0 = (blockIdx.x / ntile) * CT_TILE, j0 = (blockIdx.x % ntile) * CT_TILE;
  float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
  for (int k0 = 0; k0 < H; k0 += CT_KSTEP) {
#pragma unroll
    for (int e = 0; e < 2; ++e) {
      const int r = (t >> 5) + 8 * e, k = t & 31;      // 32 consecutive floats of one row per half wave
      const bool kin = k0 + k < H;
      ts[r][k] = kin && i0 + r < B ? text[(size_t)(i0 + r) * ldt + k0 + k] : 0.f;
      is[r][k] = kin && j0 + r < B ? image[(size_t)(j0 + r) * ldi + k0 + k] : 0.f;
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < CT_KSTEP; k += 4) {
      a0 = fmaf(ts[y][k], is[x][k], a0);
      a1 = fmaf(ts[y][k + 1], is[x][k + 1], a1);
      a2 = fmaf(ts[y][k + 2], is[x][k + 2], a2);
      a3 = fmaf(ts[y][k + 3], is[x][k + 3], a3);
    }
    __syncthreads();
  }
  const int i = i0 + y, j = j0 + x;
  if (i < B && j < B) sim[(size_t)i * lds + j] = expf(log_scale[0]) * ((a0 + a1) + (a2 + a3));
}

// one wave per row (blocks 0 .. B-1: lse_row, elements one float apart) or column (blocks B .. 2B-1: lse_col, elements lds apart);
// term[b] = lse - the diagonal element, what the loss averages
__global__ __launch_bounds__(64) void contrastive_lse_kernel(const float* __restrict__ sim, int lds, float* __restrict__ lse_row,
                                                             float* __restrict__ lse_col, float* __restrict__ term, int B) {
  const bool col = (int)blockIdx.x >= B;
  const int r = col ? blockIdx.x - B : blockIdx.x, l = threadIdx.x;
  const float* x = col ? sim + r : sim + (size_t)r * lds;
  const size_t step = col ? (size_t)lds : 1;
  float m = -INFINITY;
  for (int n = l; n < B; n += 64) m = fmaxf(m, x[n * step]);
  m = wave_max(m);
  float s = 0.f;
  for (int n = l; n < B; n += 64) s += expf(x[n * step] - m);
  s = wave_sum(s);
  if (l == 0) {
    const float lse = m + logf(s);
    (col ? lse_col : lse_row)[r] = lse;
    term[blockIdx.x] = lse - sim[(size_t)r * lds + r];
  }
}

__global__ __launch_bounds__(64) void contrastive_loss_kernel(const float* __restrict__ term, int B, float* __restrict__ loss) {
  float r = 0.f, c = 0.f;
  for (int n = threadIdx.x; n < B; n += 64) { r += term[n]; c += term[B + n]; }
  r = wave_sum(r);
  c = wave_sum(c);
  if (threadIdx.x == 0) loss[0] = 0.5f * (r / (float)B + c / (float)B);
}

// one wave per row i: G[i][0 .. B-1] (dense, B floats a row) and part[i] = sum_j G[i][j] sim[i][j]
__global__ __launch_bounds__(64) void contrastive_g_kernel(const float* __restrict__ sim, int lds, const float* __restrict__ lse_row,
                                                           const float* __restrict__ lse_col, const float* __restrict__ dloss,
                                                           float* __restrict__ G, float* __restrict__ part, int B) {
  const int i = blockIdx.x, l = threadIdx.x;
  const float c = dloss[0] * (0.5f / (float)B), lr = lse_row[i];
  float acc = 0.f;
  for (int j = l; j < B; j += 64) {
    const float v = sim[(size_t)i * lds + j];
    const float g = c * ((expf(v - lr) + expf(v - lse_col[j])) - (i == j ? 2.f : 0.f));
    G[(size_t)i * B + j] = g;
    acc = fmaf(g, v, acc);
  }
  acc = wave_sum(acc);
  if (l == 0) part[i] = acc;
}

__global__ __launch_bounds__(64) void contrastive_dscale_kernel(const float* __restrict__ part, int B, float* __restrict__ dlog_scale,
                                                                int accumulate) {
  float s = 0.f;
  for (int n = threadIdx.x; n < B; n += 64) s += part[n];
  s = wave_sum(s);
  if (threadIdx.x == 0) dlog_scale[0] = accumulate ? dlog_scale[0] + s : s;
}

// blockIdx.z = 0: dtext[r][k] = s sum_n G[r][n] image[n][k]; 1: dimage[r][k] = s sum_n G[n][r] text[n][k].  One thread per (r, k): the G
// element is the same for the whole workgroup, the operand row is read 256 consecutive floats at a time.
__global__ __launch_bounds__(CT_THREADS) void contrastive_dembed_kernel(const float* __restrict__ G, const float* __restrict__ text, int ldt,
                                                                        const float* __restrict__ image, int ldi,
                                                                        const float* __restrict__ log_scale, float* __restrict__ dtext,
                                                                        int lddt, float* __restrict__ dimage, int lddi, int B, int H) {
  const int r = blockIdx.x, k = blockIdx.y * CT_THREADS + threadIdx.x;
  if (k >= H) return;
  const bool tr = blockIdx.z != 0;
  const float* src = (tr ? text : image) + k;
  const size_t lsrc = tr ? ldt : ldi;
  const float* g = tr ? G + r : G + (size_t)r * B;
  const size_t gstep = tr ? (size_t)B : 1;
  float a[4] = {0.f, 0.f, 0.f, 0.f};
  int n = 0;
  for (; n + 4 <= B; n += 4) {
#pragma unroll
    for (int e = 0; e < 4; ++e) a[e] = fmaf(g[(n + e) * gstep], src[(n + e) * lsrc], a[e]);
  }
#pragma unroll
  for (int e = 0; e < 3; ++e)
    if (n + e < B) a[e] = fmaf(g[(n + e) * gstep], src[(n + e) * lsrc], a[e]);
  const float v = expf(log_scale[0]) * ((a[0] + a[1]) + (a[2] + a[3]));
  if (tr) dimage[(size_t)r * lddi + k] = v;
  else dtext[(size_t)r * lddt + k] = v;
}

inline size_t ct_round(size_t b) { return (b + 255) & ~(size_t)255; }
// the flattened grid of 16 x 16 tiles has to fit an int
inline bool ct_batch_ok(int B) { const size_t nt = ((size_t)B + CT_TILE - 1) / CT_TILE; return B >= 1 && nt * nt <= (size_t)INT_MAX; }

}  // namespace

// backward: G [B, B] and part [B]; forward: term [2 B], never more than that
extern "C" size_t ia_contrastive_workspace_bytes(int B) {
  if (B <= 0) return 0;
  return ct_round(((size_t)B * B + B) * sizeof(float));
}

extern "C" int ia_contrastive_fwd(const float* text, int ldt, const float* image, int ldi, const float* log_scale, float* sim, int lds,
                                  float* lse_row, float* lse_col, float* loss, int B, int H, void* workspace, size_t workspace_bytes,
                                  hipStream_t stream) {
  (void)hipGetLastError();
  if (!text || !image || !log_scale || !sim || !lse_row || !lse_col || !loss || B < 1 || H < 1 || ldt < H || ldi < H || lds < B)
    return IA_ERR_ARG;
  if (!ct_batch_ok(B) || ((uintptr_t)workspace & 3)) return IA_ERR_ARG;
  if (!workspace || workspace_bytes < ia_contrastive_workspace_bytes(B)) return IA_ERR_WORKSPACE;
  float* term = (float*)workspace;
  const int ntile = (B + CT_TILE - 1) / CT_TILE;
  contrastive_sim_kernel<<<ntile * ntile, CT_THREADS, 0, stream>>>(text, ldt, image, ldi, log_scale, sim, lds, B, H, ntile);
  contrastive_lse_kernel<<<2 * B, 64, 0, stream>>>(sim, lds, lse_row, lse_col, term, B);
  contrastive_loss_kernel<<<1, 64, 0, stream>>>(term, B, loss);
  return ia_check_launch();
}

extern "C" int ia_contrastive_bwd(const float* text, int ldt, const float* image, int ldi, const float* log_scale, const float* sim, int lds,
                                  const float* lse_row, const float* lse_col, const float* dloss, float* dtext, int lddt, float* dimage,
                                  int lddi, float* dlog_scale, int accumulate_dlog_scale, int B, int H, void* workspace,
                                  size_t workspace_bytes, hipStream_t stream) {
  (void)hipGetLastError();
  if (!text || !image || !log_scale || !sim || !lse_row || !lse_col || !dloss || !dtext || !dimage || !dlog_scale || B < 1 || H < 1 ||
      ldt < H || ldi < H || lds < B || lddt < H || lddi < H)
    return IA_ERR_ARG;
  if (!ct_batch_ok(B) || ((uintptr_t)workspace & 3)) return IA_ERR_ARG;
  if (!workspace || workspace_bytes < ia_contrastive_workspace_bytes(B)) return IA_ERR_WORKSPACE;
  float* G = (float*)workspace;
  float* part = G + (size_t)B * B;
  const int kblocks = (H + CT_THREADS - 1) / CT_THREADS;
  if (kblocks > 65535) return IA_ERR_ARG;
  contrastive_g_kernel<<<B, 64, 0, stream>>>(sim, lds, lse_row, lse_col, dloss, G, part, B);
  contrastive_dscale_kernel<<<1, 64, 0, stream>>>(part, B, dlog_scale, accumulate_dlog_scale);
  contrastive_dembed_kernel<<<dim3(B, kblocks, 2), CT_THREADS, 0, stream>>>(G, text, ldt, image, ldi, log_scale, dtext, lddt, dimage, lddi, B, H);
  return ia_check_launch();
}
