// Optimiser step over the flat parameter arena (HBM-bound: 28 B/param read+write + 2 B shadow), gfx950.
//
// The reference builds torch.optim.AdamW with two parameter groups (weight decay everywhere except
// names containing "bias" / "LayerNorm.weight", finetune_multimodal.py:296-308) and steps it once per
// optimiser step (:460-468).  Here all fp32 master parameters, their gradients and both Adam moments
// live in four flat arenas with identical element offsets; one launch walks a static chunk table
// {offset, count, weight-decay flag} and also refreshes the bf16 shadow copy the GEMMs read.
#include "common.h"
#include "../../include/itemalign.h"
#include <cstdio>

namespace {

struct Chunk { uint32_t offset_lo; uint32_t offset_hi; uint32_t count; uint32_t decay; };

// PyTorch AdamW update order: p *= 1 - lr*wd ; m,v update ; p -= (lr/bc1) * m / (sqrt(v)/sqrt(bc2) + eps)
__global__ __launch_bounds__(256) void adamw_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                                    float* __restrict__ v, bf16* __restrict__ shadow, const Chunk* __restrict__ table,
                                                    float lr, float beta1, float beta2, float eps, float wd, float bc1, float bc2_sqrt,
                                                    float grad_scale) {
  const Chunk c = table[blockIdx.x];
  const size_t base = ((size_t)c.offset_hi << 32) | c.offset_lo;
  const float decay = c.decay ? 1.f - lr * wd : 1.f;
  const float step = lr / bc1;
  for (uint32_t i = threadIdx.x * 4; i < c.count; i += 256 * 4) {
    const size_t e = base + i;
    if (i + 4 <= c.count) {
      f32x4 pp = *reinterpret_cast<f32x4*>(p + e);
      const f32x4 gg = *reinterpret_cast<const f32x4*>(g + e);
      f32x4 mm = *reinterpret_cast<f32x4*>(m + e), vv = *reinterpret_cast<f32x4*>(v + e);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const float gr = gg[j] * grad_scale;
        pp[j] *= decay;
        mm[j] = beta1 * mm[j] + (1.f - beta1) * gr;
        vv[j] = beta2 * vv[j] + (1.f - beta2) * gr * gr;
        pp[j] -= step * mm[j] / (sqrtf(vv[j]) / bc2_sqrt + eps);
      }
      *reinterpret_cast<f32x4*>(p + e) = pp;
      *reinterpret_cast<f32x4*>(m + e) = mm;
      *reinterpret_cast<f32x4*>(v + e) = vv;
      if (shadow) {
        bf16x4 s = {f2bf(pp[0]), f2bf(pp[1]), f2bf(pp[2]), f2bf(pp[3])};
        *reinterpret_cast<bf16x4*>(shadow + e) = s;
      }
    } else {
      for (uint32_t j = i; j < c.count; ++j) {
        const size_t ee = base + j;
        const float gr = g[ee] * grad_scale;
        float pp = p[ee] * decay;
        const float mm = beta1 * m[ee] + (1.f - beta1) * gr;
        const float vv = beta2 * v[ee] + (1.f - beta2) * gr * gr;
        pp -= step * mm / (sqrtf(vv) / bc2_sqrt + eps);
        p[ee] = pp; m[ee] = mm; v[ee] = vv;
        if (shadow) shadow[ee] = f2bf(pp);
      }
    }
  }
}

// ---- LAMB (You et al., ICLR 2020) over the same arenas: the Adam direction u, rescaled per parameter tensor by r_T = ||w_T|| / ||u_T||.
// The update needs two norms per tensor before a weight may move, so the step is a short chain of launches on one stream:
//   lamb_gsq_kernel     (clipping only) chunk c -> partial sum of g^2                                        4 B / parameter read
//   lamb_scale_kernel   (clipping only) the partials, in fp64 -> the gradient factor s, a float in the workspace
//   lamb_moments_kernel chunk c: m, v updated and stored, u formed, partial sums of w^2 and u^2           16 B read, 8 B written
//   lamb_ratio_kernel   tensor T: its chunks' partials, in fp64 -> r_T, also written once per chunk of T
//   lamb_apply_kernel   chunk c: u recomputed from the stored m, v and w; w -= lr r_T u; bf16 shadow       12 B read, 6 B written
// No atomics and no value read back by the host.  Within a chunk the sum is fp32 in a fixed order (each thread over its elements in
// ascending order, a DPP tree inside the wave, the four waves in order); across chunks it is fp64 in an order that only depends on the
// tables -- never on the grid -- so two runs, or two data-parallel ranks holding the same gradients, produce the same bits.
struct LambTensor { uint32_t first_chunk; uint32_t n_chunks; uint32_t flags; };

// total over the 256 threads of a workgroup (red: 4 floats of LDS); every thread must arrive
IA_DEV float block_sum256(float v, float* red) {
  v = wave_sum(v);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  const float r = (red[0] + red[1]) + (red[2] + red[3]);
  __syncthreads();
  return r;
}

// total over the NT threads of a workgroup in fp64: a fixed binary tree through LDS (red: NT doubles); the result is valid in thread 0
template <int NT>
IA_DEV double block_sum_f64(double v, double* red) {
  red[threadIdx.x] = v;
  __syncthreads();
#pragma unroll
  for (int s = NT / 2; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
    __syncthreads();
  }
  return red[0];
}

// the LAMB direction of one element: bias-corrected Adam quotient + decoupled decay.  Both passes that need u call this, so the
// apply pass recomputes exactly the bits whose norm the ratio was taken from.
IA_DEV float lamb_u(float m, float v, float w, float rbc1, float rbc2, float eps, float wd) {
  const float q = (m * rbc1) / (sqrtf(v * rbc2) + eps);
  return __builtin_fmaf(wd, w, q);
}

__global__ __launch_bounds__(256) void lamb_gsq_kernel(const float* __restrict__ g, const Chunk* __restrict__ table, float* __restrict__ part) {
  __shared__ float red[4];
  const Chunk c = table[blockIdx.x];
  const size_t base = ((size_t)c.offset_hi << 32) | c.offset_lo;
  float acc = 0.f;
  for (uint32_t i = threadIdx.x * 4; i < c.count; i += 256 * 4) {
    const size_t e = base + i;
    if (i + 4 <= c.count) {
      const f32x4 gg = *reinterpret_cast<const f32x4*>(g + e);
#pragma unroll
      for (int j = 0; j < 4; ++j) acc = __builtin_fmaf(gg[j], gg[j], acc);
    } else {
      for (uint32_t j = i; j < c.count; ++j) acc = __builtin_fmaf(g[base + j], g[base + j], acc);
    }
  }
  const float total = block_sum256(acc, red);
  if (threadIdx.x == 0) part[blockIdx.x] = total;
}

// s = grad_scale * min(1, max_norm / (grad_scale * ||g|| + 1e-6)): train.clipped_adamw_step's factor, formed on the device
__global__ __launch_bounds__(1024) void lamb_scale_kernel(const float* __restrict__ part, int n_chunks, float grad_scale, float max_norm,
                                                          float* __restrict__ s_out) {
  __shared__ double red[1024];
  double acc = 0.0;
  for (int i = threadIdx.x; i < n_chunks; i += 1024) acc += (double)part[i];
  const double total = block_sum_f64<1024>(acc, red);
  if (threadIdx.x == 0) {
    const double norm = sqrt(total) * (double)grad_scale;
    const double f = fmin(1.0, (double)max_norm / (norm + 1e-6));
    *s_out = (float)((double)grad_scale * f);
  }
}

__global__ __launch_bounds__(256) void lamb_moments_kernel(const float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                                           float* __restrict__ v, const Chunk* __restrict__ table,
                                                           const float* __restrict__ s_ptr, float grad_scale, float beta1, float beta2,
                                                           float eps, float wd, float rbc1, float rbc2, float* __restrict__ wsq,
                                                           float* __restrict__ usq, float* __restrict__ rchunk) {
  __shared__ float red[4];
  const Chunk c = table[blockIdx.x];
  const size_t base = ((size_t)c.offset_hi << 32) | c.offset_lo;
  const float s = s_ptr ? *s_ptr : grad_scale;
  const float cwd = c.decay ? wd : 0.f;
  const float omb1 = 1.f - beta1, omb2 = 1.f - beta2;
  float aw = 0.f, au = 0.f;
  for (uint32_t i = threadIdx.x * 4; i < c.count; i += 256 * 4) {
    const size_t e = base + i;
    if (i + 4 <= c.count) {
      const f32x4 pp = *reinterpret_cast<const f32x4*>(p + e);
      const f32x4 gg = *reinterpret_cast<const f32x4*>(g + e);
      f32x4 mm = *reinterpret_cast<f32x4*>(m + e), vv = *reinterpret_cast<f32x4*>(v + e);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const float gr = gg[j] * s;
        mm[j] = __builtin_fmaf(beta1, mm[j], omb1 * gr);
        vv[j] = __builtin_fmaf(beta2, vv[j], omb2 * (gr * gr));
        const float u = lamb_u(mm[j], vv[j], pp[j], rbc1, rbc2, eps, cwd);
        aw = __builtin_fmaf(pp[j], pp[j], aw);
        au = __builtin_fmaf(u, u, au);
      }
      *reinterpret_cast<f32x4*>(m + e) = mm;
      *reinterpret_cast<f32x4*>(v + e) = vv;
    } else {
      for (uint32_t j = i; j < c.count; ++j) {
        const size_t ee = base + j;
        const float gr = g[ee] * s, pp = p[ee];
        const float mm = __builtin_fmaf(beta1, m[ee], omb1 * gr);
        const float vv = __builtin_fmaf(beta2, v[ee], omb2 * (gr * gr));
        const float u = lamb_u(mm, vv, pp, rbc1, rbc2, eps, cwd);
        aw = __builtin_fmaf(pp, pp, aw);
        au = __builtin_fmaf(u, u, au);
        m[ee] = mm; v[ee] = vv;
      }
    }
  }
  const float tw = block_sum256(aw, red);
  const float tu = block_sum256(au, red);
  if (threadIdx.x == 0) {
    wsq[blockIdx.x] = tw;
    usq[blockIdx.x] = tu;
    rchunk[blockIdx.x] = 1.f;      // a chunk no tensor of the table claims takes the plain direction
  }
}

// one workgroup per tensor: thread t adds the partials of chunks t, t + 256, ... of the tensor in ascending order, then a fixed tree
__global__ __launch_bounds__(256) void lamb_ratio_kernel(const LambTensor* __restrict__ tensors, int n_chunks_total,
                                                         const float* __restrict__ wsq, const float* __restrict__ usq,
                                                         float* __restrict__ ratio, float* __restrict__ rchunk) {
  __shared__ double red[256];
  __shared__ float r_lds;
  const LambTensor t = tensors[blockIdx.x];
  const bool ok = t.n_chunks > 0 && t.first_chunk < (uint32_t)n_chunks_total && t.n_chunks <= (uint32_t)n_chunks_total - t.first_chunk;
  float r = 1.f;
  if (ok && (t.flags & IA_LAMB_ADAPT)) {      // block-uniform
    double aw = 0.0, au = 0.0;
    for (uint32_t i = threadIdx.x; i < t.n_chunks; i += 256) {
      aw += (double)wsq[t.first_chunk + i];
      au += (double)usq[t.first_chunk + i];
    }
    const double w2 = block_sum_f64<256>(aw, red);
    __syncthreads();
    const double u2 = block_sum_f64<256>(au, red);
    if (threadIdx.x == 0) r_lds = (w2 > 0.0 && u2 > 0.0) ? (float)(sqrt(w2) / sqrt(u2)) : 1.f;
    __syncthreads();
    r = r_lds;
  }
  if (threadIdx.x == 0) ratio[blockIdx.x] = r;
  if (ok)
    for (uint32_t i = threadIdx.x; i < t.n_chunks; i += 256) rchunk[t.first_chunk + i] = r;
}

__global__ __launch_bounds__(256) void lamb_apply_kernel(float* __restrict__ p, const float* __restrict__ m, const float* __restrict__ v,
                                                         bf16* __restrict__ shadow, const Chunk* __restrict__ table,
                                                         const float* __restrict__ rchunk, float lr, float eps, float wd, float rbc1,
                                                         float rbc2) {
  const Chunk c = table[blockIdx.x];
  const size_t base = ((size_t)c.offset_hi << 32) | c.offset_lo;
  const float cwd = c.decay ? wd : 0.f;
  const float nstep = -(lr * rchunk[blockIdx.x]);
  for (uint32_t i = threadIdx.x * 4; i < c.count; i += 256 * 4) {
    const size_t e = base + i;
    if (i + 4 <= c.count) {
      f32x4 pp = *reinterpret_cast<f32x4*>(p + e);
      const f32x4 mm = *reinterpret_cast<const f32x4*>(m + e), vv = *reinterpret_cast<const f32x4*>(v + e);
#pragma unroll
      for (int j = 0; j < 4; ++j) pp[j] = __builtin_fmaf(nstep, lamb_u(mm[j], vv[j], pp[j], rbc1, rbc2, eps, cwd), pp[j]);
      *reinterpret_cast<f32x4*>(p + e) = pp;
      if (shadow) {
        bf16x4 s = {f2bf(pp[0]), f2bf(pp[1]), f2bf(pp[2]), f2bf(pp[3])};
        *reinterpret_cast<bf16x4*>(shadow + e) = s;
      }
    } else {
      for (uint32_t j = i; j < c.count; ++j) {
        const size_t ee = base + j;
        const float pp = __builtin_fmaf(nstep, lamb_u(m[ee], v[ee], p[ee], rbc1, rbc2, eps, cwd), p[ee]);
        p[ee] = pp;
        if (shadow) shadow[ee] = f2bf(pp);
      }
    }
  }
}

__global__ __launch_bounds__(256) void cast_f32_bf16_kernel(const float* __restrict__ src, bf16* __restrict__ dst, size_t n) {
  for (size_t i = ((size_t)blockIdx.x * 256 + threadIdx.x) * 4; i < n; i += (size_t)gridDim.x * 256 * 4) {
    if (i + 4 <= n) {
      const f32x4 a = *reinterpret_cast<const f32x4*>(src + i);
      bf16x4 o = {f2bf(a[0]), f2bf(a[1]), f2bf(a[2]), f2bf(a[3])};
      *reinterpret_cast<bf16x4*>(dst + i) = o;
    } else {
      for (size_t j = i; j < n; ++j) dst[j] = f2bf(src[j]);
    }
  }
}

__global__ __launch_bounds__(256) void cast_bf16_f32_kernel(const bf16* __restrict__ src, float* __restrict__ dst, size_t n) {
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) dst[i] = bf2f(src[i]);
}

// dst[c][r] = src[r][c] for every matrix of the table: 64 x 64 tiles through LDS (both sides move 128-byte rows), one workgroup per tile
struct TransposeEntry { uint32_t offset_lo; uint32_t offset_hi; uint32_t rows; uint32_t cols; };
__global__ __launch_bounds__(256) void transpose_batched_kernel(const bf16* __restrict__ src, bf16* __restrict__ dst,
                                                                const TransposeEntry* __restrict__ table) {
  __shared__ bf16 tile[64][66];
  const TransposeEntry e = table[blockIdx.y];
  const uint32_t tiles_c = (e.cols + 63) / 64, tiles_r = (e.rows + 63) / 64;
  if (blockIdx.x >= tiles_c * tiles_r) return;
  const size_t base = ((size_t)e.offset_hi << 32) | e.offset_lo;
  const uint32_t r0 = (blockIdx.x / tiles_c) * 64, c0 = (blockIdx.x % tiles_c) * 64;
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;              // 32 lanes x 2 columns, 8 row groups
  for (int i = ty; i < 64; i += 8) {
    const uint32_t r = r0 + i, c = c0 + 2 * tx;
    bf16 a = f2bf(0.f), b = f2bf(0.f);
    if (r < e.rows && c < e.cols) a = src[base + (size_t)r * e.cols + c];
    if (r < e.rows && c + 1 < e.cols) b = src[base + (size_t)r * e.cols + c + 1];
    tile[i][2 * tx] = a; tile[i][2 * tx + 1] = b;
  }
  __syncthreads();
  for (int i = ty; i < 64; i += 8) {
    const uint32_t c = c0 + i, r = r0 + 2 * tx;                          // output row = source column
    if (c < e.cols && r < e.rows) dst[base + (size_t)c * e.rows + r] = tile[2 * tx][i];
    if (c < e.cols && r + 1 < e.rows) dst[base + (size_t)c * e.rows + r + 1] = tile[2 * tx + 1][i];
  }
}

}  // namespace

// Transposed bf16 copies of 2-D weights (the data-gradient GEMMs dx = dy W read W^T k-contiguously: the faster operand form).
// table: device array of n {offset_lo, offset_hi, rows, cols} (element offsets into src / dst, the same on both sides);
// dst[offset .. offset + rows*cols) receives the [cols, rows] transpose of src's [rows, cols] matrix.  max_tiles = the largest
// ceil(rows/64) * ceil(cols/64) of the table.
extern "C" int ia_transpose_bf16_batched(const void* src, void* dst, const void* table, int n, int max_tiles, hipStream_t stream) {
  (void)hipGetLastError();
  if (!src || !dst || !table || n <= 0 || max_tiles <= 0 || n > 65535) return IA_ERR_ARG;
  hipLaunchKernelGGL(transpose_batched_kernel, dim3(max_tiles, n), dim3(256), 0, stream, (const bf16*)src, (bf16*)dst, (const TransposeEntry*)table);
  return ia_check_launch();
}

// table: device array of n_chunks {offset_lo, offset_hi, count (<= 4096, offsets 4-element aligned), decay}.
extern "C" int ia_adamw_flat(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, void* shadow_bf16,
                             const void* chunk_table, int n_chunks, float lr, float beta1, float beta2, float eps, float weight_decay,
                             int step, float grad_scale, hipStream_t stream) {
  (void)hipGetLastError();  // drop stale status left by unrelated runtime calls (e.g. hipEventQuery -> NotReady)
  if (!params || !grads || !exp_avg || !exp_avg_sq || !chunk_table || n_chunks <= 0 || step <= 0) return IA_ERR_ARG;
  const float bc1 = 1.f - powf(beta1, (float)step);
  const float bc2 = 1.f - powf(beta2, (float)step);
  hipLaunchKernelGGL(adamw_kernel, dim3(n_chunks), dim3(256), 0, stream, params, grads, exp_avg, exp_avg_sq, (bf16*)shadow_bf16,
                     (const Chunk*)chunk_table, lr, beta1, beta2, eps, weight_decay, bc1, sqrtf(bc2), grad_scale);
  return ia_check_launch();
}

// workspace: [0, 16) the gradient factor s (one float); [16, 16 + 4 n_tensors) r_T of the last step, one float per tensor in table
// order; then, 16-byte aligned, three float arrays of n_chunks (partial w^2 -- g^2 before it --, partial u^2, r per chunk)
static size_t lamb_ratio_bytes(int n_tensors) { return ((size_t)n_tensors * 4 + 15) / 16 * 16; }

extern "C" size_t ia_lamb_workspace_bytes(int n_chunks, int n_tensors) {
  if (n_chunks <= 0 || n_tensors <= 0) return 0;
  return 16 + lamb_ratio_bytes(n_tensors) + (size_t)n_chunks * 3 * 4;
}

// One LAMB step (the definition: DESIGN.md "LAMB").  chunk_table as for ia_adamw_flat (its decay word selects weight_decay);
// tensor_table: device array of n_tensors {first_chunk, n_chunks, flags (IA_LAMB_ADAPT)}, the chunks of a tensor adjacent and ascending.
// max_grad_norm <= 0: no clipping, the gradient factor is grad_scale and the gradient arena is read once.
extern "C" int ia_lamb_flat(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, void* shadow_bf16,
                            const void* chunk_table, int n_chunks, const void* tensor_table, int n_tensors, float lr, float beta1,
                            float beta2, float eps, float weight_decay, int step, float grad_scale, float max_grad_norm, void* workspace,
                            size_t workspace_bytes, hipStream_t stream) {
  (void)hipGetLastError();  // drop stale status left by unrelated runtime calls (e.g. hipEventQuery -> NotReady)
  if (!params || !grads || !exp_avg || !exp_avg_sq || !chunk_table || !tensor_table || n_chunks <= 0 || n_tensors <= 0 || step <= 0)
    return IA_ERR_ARG;
  if (!workspace || workspace_bytes < ia_lamb_workspace_bytes(n_chunks, n_tensors) || ((uintptr_t)workspace & 15)) return IA_ERR_WORKSPACE;
  float* s_dev = (float*)workspace;
  float* ratio = (float*)((char*)workspace + 16);
  float* wsq = (float*)((char*)workspace + 16 + lamb_ratio_bytes(n_tensors));
  float* usq = wsq + n_chunks;
  float* rchunk = usq + n_chunks;
  // 1 / (1 - beta^t) in fp64 from the fp32 betas the kernels use, rounded once
  const float rbc1 = (float)(1.0 / (1.0 - pow((double)beta1, (double)step)));
  const float rbc2 = (float)(1.0 / (1.0 - pow((double)beta2, (double)step)));
  const Chunk* chunks = (const Chunk*)chunk_table;
  const bool clip = max_grad_norm > 0.f;
  if (clip) {
    hipLaunchKernelGGL(lamb_gsq_kernel, dim3(n_chunks), dim3(256), 0, stream, grads, chunks, wsq);
    hipLaunchKernelGGL(lamb_scale_kernel, dim3(1), dim3(1024), 0, stream, (const float*)wsq, n_chunks, grad_scale, max_grad_norm, s_dev);
  }
  hipLaunchKernelGGL(lamb_moments_kernel, dim3(n_chunks), dim3(256), 0, stream, (const float*)params, grads, exp_avg, exp_avg_sq, chunks,
                     clip ? (const float*)s_dev : (const float*)nullptr, grad_scale, beta1, beta2, eps, weight_decay, rbc1, rbc2, wsq, usq,
                     rchunk);
  hipLaunchKernelGGL(lamb_ratio_kernel, dim3(n_tensors), dim3(256), 0, stream, (const LambTensor*)tensor_table, n_chunks,
                     (const float*)wsq, (const float*)usq, ratio, rchunk);
  hipLaunchKernelGGL(lamb_apply_kernel, dim3(n_chunks), dim3(256), 0, stream, params, (const float*)exp_avg, (const float*)exp_avg_sq,
                     (bf16*)shadow_bf16, chunks, (const float*)rchunk, lr, eps, weight_decay, rbc1, rbc2);
  return ia_check_launch();
}

extern "C" int ia_cast_f32_to_bf16(const float* src, void* dst, size_t n, hipStream_t stream) {
  (void)hipGetLastError();  // drop stale status left by unrelated runtime calls (e.g. hipEventQuery -> NotReady)
  if (!src || !dst || n == 0) return IA_ERR_ARG;
  size_t g = (n / 4 + 255) / 256; if (g > 8192) g = 8192; if (g == 0) g = 1;
  hipLaunchKernelGGL(cast_f32_bf16_kernel, dim3((int)g), dim3(256), 0, stream, src, (bf16*)dst, n);
  return ia_check_launch();
}

extern "C" int ia_cast_bf16_to_f32(const void* src, float* dst, size_t n, hipStream_t stream) {
  (void)hipGetLastError();  // drop stale status left by unrelated runtime calls (e.g. hipEventQuery -> NotReady)
  if (!src || !dst || n == 0) return IA_ERR_ARG;
  size_t g = (n + 255) / 256; if (g > 8192) g = 8192;
  hipLaunchKernelGGL(cast_bf16_f32_kernel, dim3((int)g), dim3(256), 0, stream, (const bf16*)src, dst, n);
  return ia_check_launch();
}

extern "C" const char* ia_strerror(int code) {
  switch (code) {
    case IA_OK: return "ok";
    case IA_ERR_ARG: return "invalid argument (null pointer, shape or alignment)";
    case IA_ERR_LAUNCH: {
      static char buf[256];
      snprintf(buf, sizeof buf, "HIP kernel launch failed: %s", hipGetErrorString(g_ia_last_hip_error));
      return buf;
    }
    case IA_ERR_WORKSPACE: return "workspace missing or too small";
    case IA_ERR_UNSUPPORTED: return "unsupported operand layout / epilogue combination";
  }
  return "unknown error";
}

extern "C" int ia_abi_version(void) { return IA_ABI_VERSION; }
