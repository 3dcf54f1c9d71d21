// Cross-entropy over vocabulary logits (the masked-LM loss of BertForPreTraining), gfx950.
//
//   ia_vocab_ce_fwd : lse[r] = log sum_j exp(x[r][j]), loss_row[r] = lse[r] - x[r][label_r], loss = {mean over the labelled rows, their
//                     count} -- nn.CrossEntropyLoss(ignore_index=-1) on [M, V] fp32 logits (reference bert_pretrain.py:564-569)
//   ia_vocab_ce_bwd : dlogits[r][j] = bf16((exp(x[r][j] - lse[r]) - [j == label_r]) * dloss / n_live), pad columns V..ldg-1 zeros: the A
//                     operand of the hidden-gradient GEMM (k-contiguous) and of the table-gradient GEMM (k-strided) as it leaves
//
// Memory-bound row work, one workgroup of four waves per row.  A row of 21 128 fp32 logits is 84 KB: the forward reads it once from HBM
// for the maximum and once more out of L2 for the sum, the backward reads it once and writes 2 bytes per element -- M V 4 and
// M V (4 + 2) bytes of HBM traffic.  Nothing is kept in registers across the passes.  Rows with a negative label read nothing.
// Every sum has a fixed order (lane-strided partial sums, DPP butterfly, the four waves in order, the row partials in order): no atomics,
// two runs agree bit for bit.  expf / logf are the library functions (1 ulp), not the fast intrinsics: an argument of -80 would cost the
// v_exp_f32 form 2^-17 of relative error and the loads hide the extra instructions.
#include <math.h>
#include "common.h"

namespace {

constexpr int VCE_THREADS = 256;      // four waves per row
constexpr int VCE_ROWS_PER_PART = 1024;   // rows summed by one workgroup of the first reduction stage

// the four waves' values combined in wave order; every thread gets the result.  `slot` is 4 floats of LDS per use.
IA_DEV float block_sum(float v, float* slot) {
  v = wave_sum(v);
  if ((threadIdx.x & 63) == 0) slot[threadIdx.x >> 6] = v;
  __syncthreads();
  return ((slot[0] + slot[1]) + slot[2]) + slot[3];
}
IA_DEV float block_max(float v, float* slot) {
  v = wave_max(v);
  if ((threadIdx.x & 63) == 0) slot[threadIdx.x >> 6] = v;
  __syncthreads();
  return fmaxf(fmaxf(slot[0], slot[1]), fmaxf(slot[2], slot[3]));
}

// fp32 summation chain of one row's sum of exponentials, as the tests count it: ceil(V / 1024) quads per thread, each quad summed as
// (e0 + e1) + (e2 + e3) [2], the tail element [1], wave_sum [4 butterfly steps + 2], the four waves [3].
__global__ __launch_bounds__(VCE_THREADS) void vocab_ce_fwd_kernel(const float* __restrict__ logits, int ld, const int64_t* __restrict__ labels,
                                                                   float* __restrict__ lse, float* __restrict__ loss_row, int V) {
  __shared__ float red[8];
  const int r = blockIdx.x, t = threadIdx.x;
  const int64_t label = labels[r];
  if (label < 0) {                   // ignored row: nothing of it is read
    if (t == 0) { lse[r] = 0.f; loss_row[r] = 0.f; }
    return;
  }
  const float* x = logits + (size_t)r * ld;
  const f32x4* x4 = reinterpret_cast<const f32x4*>(x);
  const int nq = V >> 2, tail = (nq << 2) + t;      // threads 0 .. V % 4 - 1 take one tail element each
  float m = -INFINITY;
  for (int i = t; i < nq; i += VCE_THREADS) {
    const f32x4 v = x4[i];
    m = fmaxf(m, fmaxf(fmaxf(v[0], v[1]), fmaxf(v[2], v[3])));
  }
  if (tail < V) m = fmaxf(m, x[tail]);
  m = block_max(m, red);
  float s = 0.f;
  for (int i = t; i < nq; i += VCE_THREADS) {
    const f32x4 v = x4[i];
    s += (expf(v[0] - m) + expf(v[1] - m)) + (expf(v[2] - m) + expf(v[3] - m));
  }
  if (tail < V) s += expf(x[tail] - m);
  s = block_sum(s, red + 4);
  if (t == 0) {
    const float l = m + logf(s);
    lse[r] = l;
    // a label outside the vocabulary reads nothing and poisons the mean instead of passing silently
    loss_row[r] = label < V ? l - x[label] : NAN;
  }
}

// stage 1: part[b] = {sum of loss_row, number of labelled rows} over rows 1024 b .. 1024 b + 1023; thread t adds rows t, t + 256, t + 512,
// t + 768 in that order [4], wave_sum [6], the four waves [3]
__global__ __launch_bounds__(VCE_THREADS) void vocab_ce_part_kernel(const float* __restrict__ loss_row, const int64_t* __restrict__ labels, int M,
                                                                    float* __restrict__ part) {
  __shared__ float red[8];
  const int r0 = blockIdx.x * VCE_ROWS_PER_PART, t = threadIdx.x;
  float s = 0.f, n = 0.f;
  for (int i = t; i < VCE_ROWS_PER_PART && r0 + i < M; i += VCE_THREADS)
    if (labels[r0 + i] >= 0) { s += loss_row[r0 + i]; n += 1.f; }
  s = block_sum(s, red);
  n = block_sum(n, red + 4);          // whole numbers up to 1024: exact
  if (t == 0) { part[2 * blockIdx.x] = s; part[2 * blockIdx.x + 1] = n; }
}

// stage 2 (one wave): lane l adds parts l, l + 64, ... in order, wave_sum [6]; loss = {sum / n, n}.  n is a sum of whole numbers, exact
// below 2^24 rows.  No labelled row: 0 / 0 = NaN, as torch's mean over nothing.
__global__ __launch_bounds__(64) void vocab_ce_mean_kernel(const float* __restrict__ part, int nparts, float* __restrict__ loss) {
  float s = 0.f, n = 0.f;
  for (int i = threadIdx.x; i < nparts; i += 64) { s += part[2 * i]; n += part[2 * i + 1]; }
  s = wave_sum(s);
  n = wave_sum(n);
  if (threadIdx.x == 0) { loss[0] = s / n; loss[1] = n; }
}

// one workgroup per row, 8 columns per thread and step: two 16-byte loads, one 16-byte store
__global__ __launch_bounds__(VCE_THREADS) void vocab_ce_bwd_kernel(const float* __restrict__ logits, int ld, const int64_t* __restrict__ labels,
                                                                   const float* __restrict__ lse, const float* __restrict__ loss,
                                                                   const float* __restrict__ dloss, bf16* __restrict__ dlogits, int ldg, int V) {
  const int r = blockIdx.x, t = threadIdx.x;
  const int64_t label = labels[r];
  bf16x8* g8 = reinterpret_cast<bf16x8*>(dlogits + (size_t)r * ldg);
  const int nc = ldg >> 3;
  if (label < 0 || label >= V) {      // ignored, or outside the vocabulary (the forward made the loss NaN): an exact-zero row
    bf16x8 z;
#pragma unroll
    for (int e = 0; e < 8; ++e) z[e] = f2bf(0.f);
    for (int c = t; c < nc; c += VCE_THREADS) g8[c] = z;
    return;
  }
  const float* x = logits + (size_t)r * ld;
  const float l = lse[r], scale = dloss[0] / loss[1];
  const int lab = (int)label;
  for (int c = t; c < nc; c += VCE_THREADS) {
    const int j0 = c << 3;
    float v[8];
    if (j0 + 8 <= V) {
      const f32x4 a = *reinterpret_cast<const f32x4*>(x + j0), b = *reinterpret_cast<const f32x4*>(x + j0 + 4);
#pragma unroll
      for (int e = 0; e < 4; ++e) { v[e] = a[e]; v[4 + e] = b[e]; }
    } else {
#pragma unroll
      for (int e = 0; e < 8; ++e) v[e] = j0 + e < V ? x[j0 + e] : 0.f;      // columns V .. ld - 1 are never read
    }
    bf16x8 o;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const float p = expf(v[e] - l) - (j0 + e == lab ? 1.f : 0.f);
      o[e] = f2bf(j0 + e < V ? p * scale : 0.f);
    }
    g8[c] = o;
  }
}

inline int vce_parts(int M) { return (M + VCE_ROWS_PER_PART - 1) / VCE_ROWS_PER_PART; }

}  // namespace

extern "C" size_t ia_vocab_ce_workspace_bytes(int M) {
  if (M <= 0) return 0;
  return (((size_t)vce_parts(M) * 2 * sizeof(float)) + 255) & ~(size_t)255;
}

extern "C" int ia_vocab_ce_fwd(const float* logits, int ld, const int64_t* labels, float* lse, float* loss_row, float* loss, int M, int V,
                               void* workspace, size_t workspace_bytes, hipStream_t stream) {
  (void)hipGetLastError();
  if (!logits || !labels || !lse || !loss_row || !loss || M <= 0 || V <= 0 || ld < V || (ld & 3)) return IA_ERR_ARG;
  if (((uintptr_t)logits & 15) || ((uintptr_t)workspace & 3)) return IA_ERR_ARG;
  if (!workspace || workspace_bytes < ia_vocab_ce_workspace_bytes(M)) return IA_ERR_WORKSPACE;
  float* part = (float*)workspace;
  vocab_ce_fwd_kernel<<<M, VCE_THREADS, 0, stream>>>(logits, ld, labels, lse, loss_row, V);
  vocab_ce_part_kernel<<<vce_parts(M), VCE_THREADS, 0, stream>>>(loss_row, labels, M, part);
  vocab_ce_mean_kernel<<<1, 64, 0, stream>>>(part, vce_parts(M), loss);
  return ia_check_launch();
}

extern "C" int ia_vocab_ce_bwd(const float* logits, int ld, const int64_t* labels, const float* lse, const float* loss, const float* dloss,
                               void* dlogits, int ldg, int M, int V, hipStream_t stream) {
  (void)hipGetLastError();
  if (!logits || !labels || !lse || !loss || !dloss || !dlogits || M <= 0 || V <= 0 || ld < V || (ld & 3) || ldg < V || (ldg & 7))
    return IA_ERR_ARG;
  if (((uintptr_t)logits & 15) || ((uintptr_t)dlogits & 15)) return IA_ERR_ARG;
  vocab_ce_bwd_kernel<<<M, VCE_THREADS, 0, stream>>>(logits, ld, labels, lse, loss, dloss, (bf16*)dlogits, ldg, V);
  return ia_check_launch();
}
