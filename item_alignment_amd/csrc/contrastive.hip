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
//
// The shard entries (data-parallel pre-training: this rank holds rows row_offset .. row_offset + B - 1 of a global batch of G items that
// `world` ranks share; text_g / image_g [G, H] are the gathered embeddings of all ranks, den = (float)G / (float)world):
//
//   ia_contrastive_shard_fwd : sim_t[i][j] = s text_l[i] . image_g[j] (rows row_offset + i of the global sim), sim_i[i][j] = s image_l[i]
//                              . text_g[j] (its columns row_offset + i, transposed), lse_row_l / lse_col_l their row log-sum-exps = the
//                              global lse_row / lse_col at row_offset + i, loss = 0.5 (R / den + C / den), R = sum_i (lse_row_l[i] -
//                              sim_t[i][row_offset + i]), C = sum_i (lse_col_l[i] - sim_i[i][row_offset + i]): the mean of the ranks'
//                              losses is the loss of the global batch
//   ia_contrastive_shard_bwd : with c = dloss (0.5 / den), d = row_offset + i and lse_row_g / lse_col_g [G] gathered from all ranks,
//                              Gt[i][j] = c (exp(sim_t[i][j] - lse_row_g[d]) + exp(sim_t[i][j] - lse_col_g[j]) - 2 [j == d]),
//                              Gi[i][j] = c (exp(sim_i[i][j] - lse_col_g[d]) + exp(sim_i[i][j] - lse_row_g[j]) - 2 [j == d]),
//                              dtext_l = s Gt image_g, dimage_l = s Gi text_g, dlog_scale (+)= sum_ij Gt[i][j] sim_t[i][j]: `world`
//                              times the rank's share of the global gradient, which a gradient average over the ranks turns into the
//                              global gradient.  Nothing flows back through the gathered operands: Gt's second exponential is what the
//                              other ranks' column losses send to this rank's text rows, Gi's what their row losses send to its image rows.
//
// Their chains are the ones above with the gathered length in place of B: sim n = H; the sums of exponentials, a row's part of
// dlog_scale and the dot products of dtext_l / dimage_l n = G; the two sums of the loss and the sum of the row parts n = B; den one
// rounding (exact when world divides G).  At world = 1, row_offset = 0, G = B every output is bit-identical to ia_contrastive_fwd /
// ia_contrastive_bwd: sim_i is sim transposed with the two factors of each fmaf swapped, Gi is G transposed with the two addends of
// p + q swapped, every sum takes its terms in the same order.
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

// ------------------------------------------------------------------------------------------------ the shard entries
// blockIdx.z = 0: sim_t[i][j] = s text_l[i] . image_g[j]; 1: sim_i[i][j] = s image_l[i] . text_g[j].  Tile (blockIdx.y, blockIdx.x) of
// the [B, G] rectangle, staged and summed as contrastive_sim_kernel does (the two factors of each fmaf swap in direction 1).
__global__ __launch_bounds__(CT_THREADS) void contrastive_shard_sim_kernel(const float* __restrict__ text_l, int ldtl,
                                                                           const float* __restrict__ image_l, int ldil,
                                                                           const float* __restrict__ text_g, int ldtg,
                                                                           const float* __restrict__ image_g, int ldig,
                                                                           const float* __restrict__ log_scale, float* __restrict__ sim_t,
                                                                           float* __restrict__ sim_i, int lds, int B, int G, int H) {
  __shared__ float ls[CT_TILE][CT_KSTEP + 1], gs[CT_TILE][CT_KSTEP + 1];
  const bool tr = blockIdx.z != 0;
  const float* loc = tr ? image_l : text_l;
  const float* gat = tr ? text_g : image_g;
  const size_t ldl = tr ? ldil : ldtl, ldg = tr ? ldtg : ldig;
  const int t = threadIdx.x, y = t >> 4, x = t & 15;
  const int i0 = blockIdx.y * CT_TILE, j0 = blockIdx.x * CT_TILE;
  float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
  for (int k0 = 0; k0 < H; k0 += CT_KSTEP) {
#pragma unroll
    for (int e = 0; e < 2; ++e) {
      const int r = (t >> 5) + 8 * e, k = t & 31;
      const bool kin = k0 + k < H;
      ls[r][k] = kin && i0 + r < B ? loc[(size_t)(i0 + r) * ldl + k0 + k] : 0.f;
      gs[r][k] = kin && j0 + r < G ? gat[(size_t)(j0 + r) * ldg + k0 + k] : 0.f;
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < CT_KSTEP; k += 4) {
      a0 = fmaf(ls[y][k], gs[x][k], a0);
      a1 = fmaf(ls[y][k + 1], gs[x][k + 1], a1);
      a2 = fmaf(ls[y][k + 2], gs[x][k + 2], a2);
      a3 = fmaf(ls[y][k + 3], gs[x][k + 3], a3);
    }
    __syncthreads();
  }
  const int i = i0 + y, j = j0 + x;
  if (i < B && j < G) (tr ? sim_i : sim_t)[(size_t)i * lds + j] = expf(log_scale[0]) * ((a0 + a1) + (a2 + a3));
}

// one wave per row of sim_t (blocks 0 .. B-1: the global lse_row[row_offset + r]) or of sim_i (blocks B .. 2B-1: the global
// lse_col[row_offset + r]); term[b] = lse - the row's element on the global diagonal
__global__ __launch_bounds__(64) void contrastive_shard_lse_kernel(const float* __restrict__ sim_t, const float* __restrict__ sim_i, int lds,
                                                                   float* __restrict__ lse_row_l, float* __restrict__ lse_col_l,
                                                                   float* __restrict__ term, int B, int G, int row_offset) {
  const bool col = (int)blockIdx.x >= B;
  const int r = col ? blockIdx.x - B : blockIdx.x, l = threadIdx.x;
  const float* x = (col ? sim_i : sim_t) + (size_t)r * lds;
  float m = -INFINITY;
  for (int n = l; n < G; n += 64) m = fmaxf(m, x[n]);
  m = wave_max(m);
  float s = 0.f;
  for (int n = l; n < G; n += 64) s += expf(x[n] - m);
  s = wave_sum(s);
  if (l == 0) {
    const float lse = m + logf(s);
    (col ? lse_col_l : lse_row_l)[r] = lse;
    term[blockIdx.x] = lse - x[row_offset + r];
  }
}

// den = G / world: with equal shards the rank's own batch, so that the mean of the ranks' losses is the loss of the global batch
__global__ __launch_bounds__(64) void contrastive_shard_loss_kernel(const float* __restrict__ term, int B, float den, float* __restrict__ loss) {
  float r = 0.f, c = 0.f;
  for (int n = threadIdx.x; n < B; n += 64) { r += term[n]; c += term[B + n]; }
  r = wave_sum(r);
  c = wave_sum(c);
  if (threadIdx.x == 0) loss[0] = 0.5f * (r / den + c / den);
}

// one wave per local row i.  blockIdx.y = 0: Gt[i][j] from sim_t, its own lse = lse_row_g[row_offset + i], the other lse_col_g[j],
// and part[i] = sum_j Gt[i][j] sim_t[i][j]; 1: Gi[i][j] from sim_i with the two lse vectors swapped, no part (dlog_scale is taken from
// the text direction alone: the ranks together count every element of the global matrix once).  Gt, Gi dense [B, G].
__global__ __launch_bounds__(64) void contrastive_shard_g_kernel(const float* __restrict__ sim_t, const float* __restrict__ sim_i, int lds,
                                                                 const float* __restrict__ lse_row_g, const float* __restrict__ lse_col_g,
                                                                 const float* __restrict__ dloss, float den, float* __restrict__ Gt,
                                                                 float* __restrict__ Gi, float* __restrict__ part, int B, int G,
                                                                 int row_offset) {
  const int i = blockIdx.x, l = threadIdx.x, d = row_offset + i;
  const bool tr = blockIdx.y != 0;
  const float* x = (tr ? sim_i : sim_t) + (size_t)i * lds;
  const float* other = tr ? lse_row_g : lse_col_g;
  float* g_out = (tr ? Gi : Gt) + (size_t)i * G;
  const float c = dloss[0] * (0.5f / den), own = (tr ? lse_col_g : lse_row_g)[d];
  float acc = 0.f;
  for (int j = l; j < G; j += 64) {
    const float v = x[j];
    const float g = c * ((expf(v - own) + expf(v - other[j])) - (j == d ? 2.f : 0.f));
    g_out[j] = g;
    acc = fmaf(g, v, acc);
  }
  if (tr) return;
  acc = wave_sum(acc);
  if (l == 0) part[i] = acc;
}

// blockIdx.z = 0: dtext_l[r][k] = s sum_n Gt[r][n] image_g[n][k]; 1: dimage_l[r][k] = s sum_n Gi[r][n] text_g[n][k], n over the G
// gathered rows in order, term n in accumulator n % 4
__global__ __launch_bounds__(CT_THREADS) void contrastive_shard_dembed_kernel(const float* __restrict__ Gt, const float* __restrict__ Gi,
                                                                              const float* __restrict__ text_g, int ldtg,
                                                                              const float* __restrict__ image_g, int ldig,
                                                                              const float* __restrict__ log_scale, float* __restrict__ dtext_l,
                                                                              int lddt, float* __restrict__ dimage_l, int lddi, int G, int H) {
  const int r = blockIdx.x, k = blockIdx.y * CT_THREADS + threadIdx.x;
  if (k >= H) return;
  const bool tr = blockIdx.z != 0;
  const float* src = (tr ? text_g : image_g) + k;
  const size_t lsrc = tr ? ldtg : ldig;
  const float* g = (tr ? Gi : Gt) + (size_t)r * G;
  float a[4] = {0.f, 0.f, 0.f, 0.f};
  int n = 0;
  for (; n + 4 <= G; n += 4) {
#pragma unroll
    for (int e = 0; e < 4; ++e) a[e] = fmaf(g[n + e], src[(n + e) * lsrc], a[e]);
  }
#pragma unroll
  for (int e = 0; e < 3; ++e)
    if (n + e < G) a[e] = fmaf(g[n + e], src[(n + e) * lsrc], a[e]);
  const float v = expf(log_scale[0]) * ((a[0] + a[1]) + (a[2] + a[3]));
  if (tr) dimage_l[(size_t)r * lddi + k] = v;
  else dtext_l[(size_t)r * lddt + k] = v;
}

// the shard's place in the global batch, and grids that fit: row tiles in blockIdx.y, 2 B one-wave workgroups in blockIdx.x
inline bool ct_shard_ok(int B, int G, int row_offset, int world) {
  return B >= 1 && G >= 1 && world >= 1 && row_offset >= 0 && (long long)row_offset + B <= (long long)G &&
         ((size_t)B + CT_TILE - 1) / CT_TILE <= 65535;
}

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

// backward: Gt, Gi [B, G] and part [B]; forward: term [2 B], never more than that
extern "C" size_t ia_contrastive_shard_workspace_bytes(int B, int G) {
  if (B <= 0 || G <= 0) return 0;
  return ct_round((2 * (size_t)B * G + B) * sizeof(float));
}

extern "C" int ia_contrastive_shard_fwd(const float* text_l, int ldtl, const float* image_l, int ldil, const float* text_g, int ldtg,
                                        const float* image_g, int ldig, const float* log_scale, float* sim_t, float* sim_i, int lds,
                                        float* lse_row_l, float* lse_col_l, float* loss, int B, int G, int row_offset, int world, int H,
                                        void* workspace, size_t workspace_bytes, hipStream_t stream) {
  (void)hipGetLastError();
  if (!text_l || !image_l || !text_g || !image_g || !log_scale || !sim_t || !sim_i || !lse_row_l || !lse_col_l || !loss || H < 1 ||
      !ct_shard_ok(B, G, row_offset, world) || ldtl < H || ldil < H || ldtg < H || ldig < H || lds < G)
    return IA_ERR_ARG;
  if ((uintptr_t)workspace & 3) return IA_ERR_ARG;
  if (!workspace || workspace_bytes < ia_contrastive_shard_workspace_bytes(B, G)) return IA_ERR_WORKSPACE;
  float* term = (float*)workspace;
  const float den = (float)G / (float)world;
  const dim3 tiles((G + CT_TILE - 1) / CT_TILE, (B + CT_TILE - 1) / CT_TILE, 2);
  contrastive_shard_sim_kernel<<<tiles, CT_THREADS, 0, stream>>>(text_l, ldtl, image_l, ldil, text_g, ldtg, image_g, ldig, log_scale, sim_t,
                                                                 sim_i, lds, B, G, H);
  contrastive_shard_lse_kernel<<<2 * B, 64, 0, stream>>>(sim_t, sim_i, lds, lse_row_l, lse_col_l, term, B, G, row_offset);
  contrastive_shard_loss_kernel<<<1, 64, 0, stream>>>(term, B, den, loss);
  return ia_check_launch();
}

extern "C" int ia_contrastive_shard_bwd(const float* text_g, int ldtg, const float* image_g, int ldig, const float* log_scale,
                                        const float* sim_t, const float* sim_i, int lds, const float* lse_row_g, const float* lse_col_g,
                                        const float* dloss, float* dtext_l, int lddt, float* dimage_l, int lddi, float* dlog_scale,
                                        int accumulate_dlog_scale, int B, int G, int row_offset, int world, int H, void* workspace,
                                        size_t workspace_bytes, hipStream_t stream) {
  (void)hipGetLastError();
  if (!text_g || !image_g || !log_scale || !sim_t || !sim_i || !lse_row_g || !lse_col_g || !dloss || !dtext_l || !dimage_l || !dlog_scale ||
      H < 1 || !ct_shard_ok(B, G, row_offset, world) || ldtg < H || ldig < H || lds < G || lddt < H || lddi < H)
    return IA_ERR_ARG;
  if ((uintptr_t)workspace & 3) return IA_ERR_ARG;
  if (!workspace || workspace_bytes < ia_contrastive_shard_workspace_bytes(B, G)) return IA_ERR_WORKSPACE;
  float* Gt = (float*)workspace;
  float* Gi = Gt + (size_t)B * G;
  float* part = Gi + (size_t)B * G;
  const float den = (float)G / (float)world;
  const int kblocks = (H + CT_THREADS - 1) / CT_THREADS;
  if (kblocks > 65535) return IA_ERR_ARG;
  contrastive_shard_g_kernel<<<dim3(B, 2), 64, 0, stream>>>(sim_t, sim_i, lds, lse_row_g, lse_col_g, dloss, den, Gt, Gi, part, B, G, row_offset);
  contrastive_dscale_kernel<<<1, 64, 0, stream>>>(part, B, dlog_scale, accumulate_dlog_scale);
  contrastive_shard_dembed_kernel<<<dim3(B, kblocks, 2), CT_THREADS, 0, stream>>>(Gt, Gi, text_g, ldtg, image_g, ldig, log_scale, dtext_l, lddt,
                                                                                  dimage_l, lddi, G, H);
  return ia_check_launch();
}
