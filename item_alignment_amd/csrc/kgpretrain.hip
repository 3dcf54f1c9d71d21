// Knowledge-graph pretraining of the PKGM / TransE embeddings (reference pkgm_pretrain.py over the vendored torchkge:
// models/translation.py PKGMModel / TransEModel, utils/losses.py MarginLoss, sampling.py BernoulliNegativeSampler,
// utils/training.py Trainer with torch.optim.Adam).  fp32 throughout: the tables, the projection P and every gradient.
//
// One training step (ia_kgpt_score, mode IA_KGPT_MARGIN) over B positive and B negative triples, rows j < B positive:
//   1. prep:    hn = normalize(ent[h]), tn = normalize(ent[t])                         (one wave per triple)
//   2. GEMM:    hp = hn P^T                          [2B, D] x [D, D], fp32 FMA (PKGM only)
//   3. score:   pos / neg, the hinge, the per-pair loss and the row gradients d hn, d tn, d r, d hp (one wave per pair)
//   4. GEMM:    d hn += d hp P;  dP += d hp^T hn     (split-K partials summed in a fixed order)
//   5. normbwd: d h = (d hn - hn (hn . d hn)) / |h|  (and the same for t), in place
//   6. segment sums of the 4B entity rows and the 2B relation rows into dent / drel along a stable sort by table row
//      (the piece / join scheme of embed.hip's emb_seg_* kernels): one writer per table row, no float atomics, so the
//      gradients are bit-identical from run to run.
// The GEMMs are plain LDS-tiled fp32 FMA (no reduced precision: the scores match the fp32 reference to ~1e-6).
#include "common.h"
#include "../../include/itemalign.h"

namespace {

constexpr float KGPT_EPS = 1e-12f;          // F.normalize default eps
constexpr int KGPT_PIECE = 512;             // positions of the sorted row list per segment-sum workgroup

IA_DEV int64_t kgpt_idx(const int64_t* __restrict__ a, const int64_t* __restrict__ b, int j, int B) { return j < B ? a[j] : b[j - B]; }

// ------------------------------------------------------------------------------------------------ 1. gather + normalise
// triple j < 2B: head row hsrc (h for j < B, nh after), tail row tsrc; out-of-range ids read as zero rows (the Python layer
// rejects them before the launch; this only keeps a bad id from reading outside the table)
__global__ __launch_bounds__(256) void kgpt_prep_kernel(const float* __restrict__ ent, const int64_t* __restrict__ h, const int64_t* __restrict__ nh,
                                                        const int64_t* __restrict__ t, const int64_t* __restrict__ nt, float* __restrict__ hn,
                                                        float* __restrict__ tn, float* __restrict__ norms, int B, int D, int n_ent) {
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (row >= 4 * B) return;                                   // wave-uniform
  const int j = row % (2 * B);
  const bool head = row < 2 * B;
  const int64_t e = head ? kgpt_idx(h, nh, j, B) : kgpt_idx(t, nt, j, B);
  const bool ok = e >= 0 && e < n_ent;
  const float* src = ent + (ok ? (size_t)e * D : 0);
  float* dst = (head ? hn : tn) + (size_t)j * D;
  float ss = 0.f;
  for (int c = lane * 4; c < D; c += 256) {
    const f32x4 v = ok ? *reinterpret_cast<const f32x4*>(src + c) : f32x4{0.f, 0.f, 0.f, 0.f};
    ss += v[0] * v[0] + v[1] * v[1] + v[2] * v[2] + v[3] * v[3];
  }
  const float n = sqrtf(wave_sum(ss));
  const float inv = 1.f / fmaxf(n, KGPT_EPS);
  for (int c = lane * 4; c < D; c += 256) {
    const f32x4 v = ok ? *reinterpret_cast<const f32x4*>(src + c) : f32x4{0.f, 0.f, 0.f, 0.f};
    *reinterpret_cast<f32x4*>(dst + c) = v * inv;
  }
  if (lane == 0) norms[row] = n;
}

// ------------------------------------------------------------------------------------------------ 2 / 4. fp32 GEMM
// C[m, n] (+)= sum_k A[m*sam + k*sak] * B[k*sbk + n*sbn] over k in this workgroup's split (blockIdx.z); split z writes
// C + z*split_stride.  64 x 64 tiles, 16-deep k steps through LDS, 4 x 4 outputs per thread.
constexpr int GT = 64, GK = 16;
__global__ __launch_bounds__(256) void kgpt_gemm_kernel(const float* __restrict__ A, long sam, long sak, const float* __restrict__ Bm, long sbk,
                                                        long sbn, float* __restrict__ C, int ldc, int M, int N, int K, int kchunk, long split_stride,
                                                        int accumulate) {
  __shared__ float As[GK][GT + 4];
  __shared__ float Bs[GK][GT + 4];
  const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
  const int m0 = blockIdx.y * GT, n0 = blockIdx.x * GT;
  const int k_lo = blockIdx.z * kchunk, k_hi = min(K, k_lo + kchunk);
  float acc[4][4] = {};
  for (int k0 = k_lo; k0 < k_hi; k0 += GK) {
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int e = tid + 256 * q;
      int mm, kk;
      if (sak == 1) { mm = e >> 4; kk = e & 15; } else { kk = e >> 6; mm = e & 63; }
      const int gm = m0 + mm, gk = k0 + kk;
      As[kk][mm] = (gm < M && gk < k_hi) ? A[gm * sam + gk * sak] : 0.f;
      int nn;
      if (sbk == 1) { nn = e >> 4; kk = e & 15; } else { kk = e >> 6; nn = e & 63; }
      const int gn = n0 + nn, gk2 = k0 + kk;
      Bs[kk][nn] = (gn < N && gk2 < k_hi) ? Bm[gk2 * sbk + gn * sbn] : 0.f;
    }
    __syncthreads();
#pragma unroll
    for (int kk = 0; kk < GK; ++kk) {
      const f32x4 a = *reinterpret_cast<const f32x4*>(&As[kk][ty * 4]);
      const f32x4 b = *reinterpret_cast<const f32x4*>(&Bs[kk][tx * 4]);
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int jj = 0; jj < 4; ++jj) acc[i][jj] = fmaf(a[i], b[jj], acc[i][jj]);
    }
    __syncthreads();
  }
  float* Cz = C + (size_t)blockIdx.z * split_stride;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int gm = m0 + ty * 4 + i;
    if (gm >= M) continue;
#pragma unroll
    for (int jj = 0; jj < 4; ++jj) {
      const int gn = n0 + tx * 4 + jj;
      if (gn >= N) continue;
      float* c = Cz + (size_t)gm * ldc + gn;
      *c = accumulate ? *c + acc[i][jj] : acc[i][jj];
    }
  }
}

// dst[i] += sum_{s < S} part[s * n + i], s in order
__global__ __launch_bounds__(256) void kgpt_split_sum_kernel(const float* __restrict__ part, float* __restrict__ dst, size_t n, int S) {
  for (size_t i = blockIdx.x * 256ull + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) {
    float s = 0.f;
    for (int z = 0; z < S; ++z) s += part[(size_t)z * n + i];
    dst[i] += s;
  }
}

// ------------------------------------------------------------------------------------------------ 3. scores, hinge, row grads
// PKGM: score = -d(hn + r, tn) - d(hp, r); TransE: score = -d(hn + r, tn).  d = |.|_2^2 (NORM 2) or |.|_1 (NORM 1).
// MODE 0: scores only.  MODE 1: row gradients from dpos / dneg.  MODE 2: hinge max(0, margin - pos + neg) per pair (loss_pair)
// and its gradient (dpos = -1, dneg = +1 where margin - pos + neg >= 0, torch's clamp_min backward).
template <int NORM>
IA_DEV float kgpt_dist(float x) { return NORM == 2 ? x * x : fabsf(x); }
template <int NORM>
IA_DEV float kgpt_ddist(float x) { return NORM == 2 ? 2.f * x : (float)((x > 0.f) - (x < 0.f)); }

template <int NORM, bool PROJ>
IA_DEV float kgpt_triple_score(const float* hn, const float* tn, const float* r, const float* hp, int D, int lane) {
  float s = 0.f;
  for (int c = lane * 4; c < D; c += 256) {
    const f32x4 a = *reinterpret_cast<const f32x4*>(hn + c), b = *reinterpret_cast<const f32x4*>(tn + c);
    const f32x4 rv = r ? *reinterpret_cast<const f32x4*>(r + c) : f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int q = 0; q < 4; ++q) s += kgpt_dist<NORM>(a[q] + rv[q] - b[q]);
    if (PROJ) {
      const f32x4 p = *reinterpret_cast<const f32x4*>(hp + c);
#pragma unroll
      for (int q = 0; q < 4; ++q) s += kgpt_dist<NORM>(p[q] - rv[q]);
    }
  }
  return -wave_sum(s);
}

template <int NORM, bool PROJ>
IA_DEV void kgpt_triple_grad(const float* hn, const float* tn, const float* r, const float* hp, float g, float* dhn, float* dtn, float* dr,
                             float* dhp, int D, int lane) {
  // g = d loss / d score; d score / d dist = -1
  for (int c = lane * 4; c < D; c += 256) {
    const f32x4 a = *reinterpret_cast<const f32x4*>(hn + c), b = *reinterpret_cast<const f32x4*>(tn + c);
    const f32x4 rv = r ? *reinterpret_cast<const f32x4*>(r + c) : f32x4{0.f, 0.f, 0.f, 0.f};
    f32x4 du, dw = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int q = 0; q < 4; ++q) du[q] = -g * kgpt_ddist<NORM>(a[q] + rv[q] - b[q]);
    if (PROJ) {
      const f32x4 p = *reinterpret_cast<const f32x4*>(hp + c);
#pragma unroll
      for (int q = 0; q < 4; ++q) dw[q] = -g * kgpt_ddist<NORM>(p[q] - rv[q]);
      *reinterpret_cast<f32x4*>(dhp + c) = dw;
    }
    *reinterpret_cast<f32x4*>(dhn + c) = du;
    *reinterpret_cast<f32x4*>(dtn + c) = -du;
    *reinterpret_cast<f32x4*>(dr + c) = du - dw;
  }
}

template <int NORM, bool PROJ, int MODE>
__global__ __launch_bounds__(256) void kgpt_score_kernel(const float* __restrict__ hn, const float* __restrict__ tn, const float* __restrict__ rel,
                                                         const float* __restrict__ hp, const int64_t* __restrict__ r, int B, int D, int n_rel,
                                                         float margin, const float* __restrict__ dpos, const float* __restrict__ dneg,
                                                         float* __restrict__ pos, float* __restrict__ neg, float* __restrict__ loss_pair,
                                                         float* __restrict__ dhn, float* __restrict__ dtn, float* __restrict__ dr,
                                                         float* __restrict__ dhp) {
  const int i = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (i >= B) return;                                          // wave-uniform
  const int64_t ri = r[i];
  const float* rv = (ri >= 0 && ri < n_rel) ? rel + (size_t)ri * D : nullptr;
  const size_t op = (size_t)i * D, on = (size_t)(B + i) * D;
  const float sp = kgpt_triple_score<NORM, PROJ>(hn + op, tn + op, rv, PROJ ? hp + op : nullptr, D, lane);
  const float sn = kgpt_triple_score<NORM, PROJ>(hn + on, tn + on, rv, PROJ ? hp + on : nullptr, D, lane);
  if (lane == 0) { pos[i] = sp; neg[i] = sn; }
  if (MODE == 0) return;
  float gp, gn;
  if (MODE == 1) {
    gp = dpos[i];
    gn = dneg[i];
  } else {
    const float l = margin - sp + sn;
    const bool act = l >= 0.f;
    if (lane == 0) loss_pair[i] = fmaxf(l, 0.f);
    gp = act ? -1.f : 0.f;
    gn = act ? 1.f : 0.f;
  }
  kgpt_triple_grad<NORM, PROJ>(hn + op, tn + op, rv, PROJ ? hp + op : nullptr, gp, dhn + op, dtn + op, dr + op, PROJ ? dhp + op : nullptr, D, lane);
  kgpt_triple_grad<NORM, PROJ>(hn + on, tn + on, rv, PROJ ? hp + on : nullptr, gn, dhn + on, dtn + on, dr + on, PROJ ? dhp + on : nullptr, D, lane);
}

// loss = sum of loss_pair in a fixed order (one workgroup)
__global__ __launch_bounds__(256) void kgpt_loss_sum_kernel(const float* __restrict__ loss_pair, float* __restrict__ loss, int B) {
  __shared__ float s[4];
  float v = 0.f;
  for (int i = threadIdx.x; i < B; i += 256) v += loss_pair[i];
  v = wave_sum(v);
  if ((threadIdx.x & 63) == 0) s[threadIdx.x >> 6] = v;
  __syncthreads();
  if (threadIdx.x == 0) *loss = (s[0] + s[1]) + (s[2] + s[3]);
}

// ------------------------------------------------------------------------------------------------ 5. normaliser backward
// y = x / max(|x|, eps):  dx = (dy - y (y . dy)) / |x|  (|x| >= eps),  dy / eps otherwise.  rows [0, 2B) heads, [2B, 4B) tails.
__global__ __launch_bounds__(256) void kgpt_norm_bwd_kernel(float* __restrict__ drow, const float* __restrict__ hn, const float* __restrict__ tn,
                                                            const float* __restrict__ norms, int B, int D) {
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (row >= 4 * B) return;
  const float* y = (row < 2 * B ? hn : tn) + (size_t)(row % (2 * B)) * D;
  float* g = drow + (size_t)row * D;
  float dot = 0.f;
  for (int c = lane * 4; c < D; c += 256) {
    const f32x4 a = *reinterpret_cast<const f32x4*>(y + c), b = *reinterpret_cast<const f32x4*>(g + c);
    dot += a[0] * b[0] + a[1] * b[1] + a[2] * b[2] + a[3] * b[3];
  }
  dot = wave_sum(dot);
  const float n = norms[row];
  const bool big = n >= KGPT_EPS;
  const float inv = 1.f / fmaxf(n, KGPT_EPS);
  for (int c = lane * 4; c < D; c += 256) {
    const f32x4 a = *reinterpret_cast<const f32x4*>(y + c);
    f32x4 b = *reinterpret_cast<const f32x4*>(g + c);
    b = big ? (b - a * dot) * inv : b * inv;
    *reinterpret_cast<f32x4*>(g + c) = b;
  }
}

// ------------------------------------------------------------------------------------------------ 6. deterministic segment sums
// The scheme of embed.hip's emb_seg_piece_kernel / emb_seg_join_kernel with the key of a row taken from the triple index
// arrays.  Entity rows (kind 0, 4B of them): h, nh, t, nt; relation rows (kind 1, 2B): r, r.  Keys outside [0, n_rows) get no
// gradient.  A run of equal keys inside one piece is added to the table by that piece; a run that crosses piece boundaries
// leaves its partial sums in `head` / `tail` and the piece where it starts adds them up in piece order (the relation table's
// runs are ~48 rows long at B = 32768 and span many pieces for a frequent relation).
IA_DEV long kgpt_key(int kind, int row, const int64_t* h, const int64_t* nh, const int64_t* t, const int64_t* nt, const int64_t* r, int B,
                     int n_rows) {
  int64_t k;
  if (kind == 0) k = row < 2 * B ? kgpt_idx(h, nh, row, B) : kgpt_idx(t, nt, row - 2 * B, B);
  else k = r[row % B];
  return (k >= 0 && k < n_rows) ? (long)k : -1;
}

__global__ __launch_bounds__(256) void kgpt_seg_piece_kernel(const float* __restrict__ drow, const int32_t* __restrict__ order, int kind,
                                                             const int64_t* __restrict__ h, const int64_t* __restrict__ nh,
                                                             const int64_t* __restrict__ t, const int64_t* __restrict__ nt,
                                                             const int64_t* __restrict__ r, int B, int n_rows, float* __restrict__ table,
                                                             float* __restrict__ head, float* __restrict__ tail, long* __restrict__ pkeys, int M,
                                                             int H) {
  __shared__ long s_key[KGPT_PIECE];
  __shared__ int s_row[KGPT_PIECE];
  const int p = blockIdx.x, lo = p * KGPT_PIECE, hi = min(M, lo + KGPT_PIECE), n = hi - lo;
  for (int i = threadIdx.x; i < n; i += 256) {
    const int rw = order[lo + i];
    const bool ok = rw >= 0 && rw < M;
    s_row[i] = ok ? rw : 0;
    s_key[i] = ok ? kgpt_key(kind, rw, h, nh, t, nt, r, B, n_rows) : -1;
  }
  __syncthreads();
  if (blockIdx.y == 0 && threadIdx.x == 0) { pkeys[2 * p] = s_key[0]; pkeys[2 * p + 1] = s_key[n - 1]; }
  const int col = (blockIdx.y * 256 + threadIdx.x) * 4;
  if (col >= H) return;
  auto key_at = [&](int pos) -> long {
    const int rw = order[pos];
    return (rw >= 0 && rw < M) ? kgpt_key(kind, rw, h, nh, t, nt, r, B, n_rows) : -1;
  };
  const long prev = lo > 0 ? key_at(lo - 1) : -2;
  const long next = hi < M ? key_at(hi) : -2;
  auto put = [](float* dst, const f32x4& v) { *reinterpret_cast<f32x4*>(dst) = v; };
  auto finish = [&](long key, int rs, int re, const f32x4& acc) {
    if (key < 0) return;
    if (rs == 0 && key == prev) put(head + (size_t)p * H + col, acc);
    else if (re == n && key == next) put(tail + (size_t)p * H + col, acc);
    else {
      float* tp = table + (size_t)key * H + col;
      f32x4 v = *reinterpret_cast<const f32x4*>(tp);
      v += acc;
      put(tp, v);
    }
  };
  int rs = 0;
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
  for (int i0 = 0; i0 < n; i0 += 8) {
    f32x4 v[8];
#pragma unroll
    for (int j = 0; j < 8; ++j)
      v[j] = i0 + j < n ? *reinterpret_cast<const f32x4*>(drow + (size_t)s_row[i0 + j] * H + col) : f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int i = i0 + j;
      if (i >= n) break;
      if (s_key[i] != s_key[rs]) {
        finish(s_key[rs], rs, i, acc);
        rs = i;
        acc = f32x4{0.f, 0.f, 0.f, 0.f};
      }
      acc += v[j];
    }
  }
  finish(s_key[rs], rs, n, acc);
}

__global__ __launch_bounds__(256) void kgpt_seg_join_kernel(const long* __restrict__ pkeys, float* __restrict__ table, const float* __restrict__ head,
                                                            const float* __restrict__ tail, int npieces, int H) {
  const int p = blockIdx.x;
  const int col = (blockIdx.y * 256 + threadIdx.x) * 4;
  if (col >= H || p + 1 >= npieces) return;
  const long key = pkeys[2 * p + 1];
  if (key < 0 || pkeys[2 * (p + 1)] != key) return;                             // the piece's last run ends here
  if (p > 0 && pkeys[2 * p] == key && pkeys[2 * p - 1] == key) return;           // ... and began in an earlier piece: not its owner
  f32x4 s = *reinterpret_cast<const f32x4*>(tail + (size_t)p * H + col);
  for (int q = p + 1;; ++q) {
    s += *reinterpret_cast<const f32x4*>(head + (size_t)q * H + col);
    if (q + 1 >= npieces || pkeys[2 * q + 1] != key || pkeys[2 * (q + 1)] != key) break;
  }
  float* tp = table + (size_t)key * H + col;
  f32x4 v = *reinterpret_cast<const f32x4*>(tp);
  v += s;
  *reinterpret_cast<f32x4*>(tp) = v;
}

// ------------------------------------------------------------------------------------------------ optimiser / normalise / sampler
// torch.optim.Adam (single-tensor path) with coupled L2: g' = g + wd p; m = lerp(m, g', 1 - b1); v = b2 v + (1 - b2) g'^2;
// p -= step_size * m / (sqrt(v) / bc2_sqrt + eps).  The gradient is cleared in the same pass.
__global__ __launch_bounds__(256) void kgpt_adam_l2_kernel(float* __restrict__ p, float* __restrict__ g, float* __restrict__ m, float* __restrict__ v,
                                                           size_t n, float b1, float b2, float eps, float wd, float step_size, float bc2_sqrt) {
  const float w1 = 1.f - b1, w2 = 1.f - b2;
  auto one = [&](float& pp, float& gg, float& mm, float& vv) {
    const float gr = gg + wd * pp;
    mm = mm + w1 * (gr - mm);
    vv = vv * b2 + w2 * gr * gr;
    pp = pp - step_size * (mm / (sqrtf(vv) / bc2_sqrt + eps));
    gg = 0.f;
  };
  const size_t n4 = n / 4;
  for (size_t i = blockIdx.x * 256ull + threadIdx.x; i < n4; i += (size_t)gridDim.x * 256) {
    f32x4 pp = reinterpret_cast<f32x4*>(p)[i], gg = reinterpret_cast<f32x4*>(g)[i], mm = reinterpret_cast<f32x4*>(m)[i],
          vv = reinterpret_cast<f32x4*>(v)[i];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      float a = pp[q], b = gg[q], c = mm[q], d = vv[q];
      one(a, b, c, d);
      pp[q] = a; gg[q] = b; mm[q] = c; vv[q] = d;
    }
    reinterpret_cast<f32x4*>(p)[i] = pp;
    reinterpret_cast<f32x4*>(g)[i] = gg;
    reinterpret_cast<f32x4*>(m)[i] = mm;
    reinterpret_cast<f32x4*>(v)[i] = vv;
  }
  if (blockIdx.x == 0 && threadIdx.x < (n & 3)) {
    const size_t i = n4 * 4 + threadIdx.x;
    one(p[i], g[i], m[i], v[i]);
  }
}

__global__ __launch_bounds__(256) void kgpt_row_normalize_kernel(float* __restrict__ x, int rows, int D) {
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (row >= rows) return;
  float* p = x + (size_t)row * D;
  float ss = 0.f;
  for (int c = lane * 4; c < D; c += 256) {
    const f32x4 v = *reinterpret_cast<const f32x4*>(p + c);
    ss += v[0] * v[0] + v[1] * v[1] + v[2] * v[2] + v[3] * v[3];
  }
  const float inv = 1.f / fmaxf(sqrtf(wave_sum(ss)), KGPT_EPS);
  for (int c = lane * 4; c < D; c += 256) {
    const f32x4 v = *reinterpret_cast<const f32x4*>(p + c);
    *reinterpret_cast<f32x4*>(p + c) = v * inv;
  }
}

// splitmix64 of (seed, fact, stream): counter-based, so the draw of a fact does not depend on the launch shape
IA_DEV uint64_t kgpt_mix(uint64_t x) {
  x += 0x9E3779B97F4A7C15ull;
  x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
  x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
  return x ^ (x >> 31);
}

// BernoulliNegativeSampler.corrupt_batch with n_neg = 1: the head is replaced with probability bern_probs[r], the tail otherwise,
// by randint(1, n_ent).  A relation id outside [0, n_probs) takes probability 0.5.
__global__ __launch_bounds__(256) void kgpt_corrupt_kernel(const int64_t* __restrict__ h, const int64_t* __restrict__ t, const int64_t* __restrict__ r,
                                                           int n, const float* __restrict__ probs, int n_probs, int n_ent, uint64_t seed,
                                                           int64_t* __restrict__ nh, int64_t* __restrict__ nt) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const uint64_t base = kgpt_mix(seed ^ kgpt_mix((uint64_t)i));
  const uint64_t u1 = kgpt_mix(base), u2 = kgpt_mix(base + 1);
  const int64_t ri = r[i];
  const float pr = (ri >= 0 && ri < n_probs) ? probs[ri] : 0.5f;
  const bool head = (float)(u1 >> 40) * (1.f / 16777216.f) < pr;              // 24-bit uniform in [0, 1)
  const int64_t e = 1 + (int64_t)__umul64hi(u2, (uint64_t)(n_ent - 1));      // uniform in [1, n_ent)
  nh[i] = head ? e : h[i];
  nt[i] = head ? t[i] : e;
}

inline unsigned kgpt_rows_grid(long rows) { return (unsigned)((rows + 3) / 4); }
inline size_t kgpt_pieces(long M) { return ((size_t)M + KGPT_PIECE - 1) / KGPT_PIECE; }
constexpr int KGPT_DP_SPLIT = 16;

struct KgptWs {
  float *hn, *tn, *hp, *drow_ent, *drow_rel, *dhp, *norms, *loss_pair, *head, *tail, *dp_part;
  long* pkeys;
  size_t bytes;
};

KgptWs kgpt_ws_layout(char* base, int B, int D, int use_proj) {
  KgptWs w{};
  size_t off = 0;
  auto take = [&](size_t n_floats) { float* p = base ? reinterpret_cast<float*>(base + off) : nullptr; off += ((n_floats * 4 + 255) / 256) * 256; return p; };
  const size_t rows2 = (size_t)2 * B * D;
  w.hn = take(rows2);
  w.tn = take(rows2);
  w.hp = use_proj ? take(rows2) : nullptr;
  w.dhp = use_proj ? take(rows2) : nullptr;
  w.drow_ent = take(2 * rows2);
  w.drow_rel = take(rows2);
  w.norms = take((size_t)4 * B);
  w.loss_pair = take((size_t)B);
  const size_t pieces = kgpt_pieces(4L * B);            // the entity list is the longer one
  w.head = take(pieces * D);
  w.tail = take(pieces * D);
  w.pkeys = reinterpret_cast<long*>(take(pieces * 4));  // 2 int64 per piece
  w.dp_part = use_proj ? take((size_t)KGPT_DP_SPLIT * D * D) : nullptr;
  w.bytes = off;
  return w;
}

void kgpt_gemm(const float* A, long sam, long sak, const float* Bm, long sbk, long sbn, float* C, int ldc, int M, int N, int K, int splits,
               long split_stride, int accumulate, hipStream_t stream) {
  const int kchunk = ((K + splits - 1) / splits + GK - 1) / GK * GK;
  const dim3 grid((N + GT - 1) / GT, (M + GT - 1) / GT, splits);
  hipLaunchKernelGGL(kgpt_gemm_kernel, grid, dim3(256), 0, stream, A, sam, sak, Bm, sbk, sbn, C, ldc, M, N, K, kchunk, split_stride, accumulate);
}

}  // namespace

extern "C" size_t ia_kgpt_workspace_bytes(int B, int D, int use_proj) {
  if (B <= 0 || D <= 0) return 0;
  return kgpt_ws_layout(nullptr, B, D, use_proj).bytes;
}

extern "C" int ia_kgpt_score(const float* ent, const float* rel, const float* proj, const int64_t* h, const int64_t* t, const int64_t* r,
                             const int64_t* nh, const int64_t* nt, int B, int D, int n_ent, int n_rel, int norm, int mode, float margin,
                             const float* dpos, const float* dneg, float* pos, float* neg, float* loss, const int32_t* ent_order,
                             const int32_t* rel_order, float* dent, float* drel, float* dproj, void* workspace, size_t workspace_bytes,
                             hipStream_t stream) {
  (void)hipGetLastError();  // drop stale status left by unrelated runtime calls (e.g. hipEventQuery -> NotReady)
  if (!ent || !rel || !h || !t || !r || !nh || !nt || !pos || !neg) return IA_ERR_ARG;
  if (B <= 0 || D <= 0 || (D & 3) || n_ent <= 0 || n_rel <= 0 || (norm != 1 && norm != 2) || mode < 0 || mode > 2) return IA_ERR_ARG;
  if ((long)4 * B > 0x7fffffffL / 2) return IA_ERR_ARG;
  if (mode == IA_KGPT_GRAD && (!dpos || !dneg)) return IA_ERR_ARG;
  if (mode == IA_KGPT_MARGIN && !loss) return IA_ERR_ARG;
  if (mode != IA_KGPT_SCORE && (!ent_order || !rel_order || !dent || !drel || (proj && !dproj))) return IA_ERR_ARG;
  const int use_proj = proj != nullptr;
  if (!workspace || workspace_bytes < ia_kgpt_workspace_bytes(B, D, use_proj)) return IA_ERR_WORKSPACE;
  const KgptWs w = kgpt_ws_layout((char*)workspace, B, D, use_proj);
  const dim3 blk(256);
  hipLaunchKernelGGL(kgpt_prep_kernel, dim3(kgpt_rows_grid(4L * B)), blk, 0, stream, ent, h, nh, t, nt, w.hn, w.tn, w.norms, B, D, n_ent);
  if (use_proj)   // hp[2B, D] = hn P^T
    kgpt_gemm(w.hn, D, 1, proj, 1, D, w.hp, D, 2 * B, D, D, 1, 0, 0, stream);
  float* dhn = w.drow_ent;
  float* dtn = w.drow_ent + (size_t)2 * B * D;
#define IA_S(NORM, PROJ, MODE) hipLaunchKernelGGL((kgpt_score_kernel<NORM, PROJ, MODE>), dim3(kgpt_rows_grid(B)), blk, 0, stream, w.hn, w.tn, rel, \
    w.hp, r, B, D, n_rel, margin, dpos, dneg, pos, neg, w.loss_pair, dhn, dtn, w.drow_rel, w.dhp)
#define IA_SM(NORM, PROJ) switch (mode) { case 0: IA_S(NORM, PROJ, 0); break; case 1: IA_S(NORM, PROJ, 1); break; default: IA_S(NORM, PROJ, 2); }
  if (norm == 2) { if (use_proj) { IA_SM(2, true) } else { IA_SM(2, false) } }
  else { if (use_proj) { IA_SM(1, true) } else { IA_SM(1, false) } }
#undef IA_SM
#undef IA_S
  if (mode == IA_KGPT_SCORE) return ia_check_launch();
  if (mode == IA_KGPT_MARGIN) hipLaunchKernelGGL(kgpt_loss_sum_kernel, dim3(1), blk, 0, stream, w.loss_pair, loss, B);
  if (use_proj) {
    kgpt_gemm(w.dhp, D, 1, proj, D, 1, dhn, D, 2 * B, D, D, 1, 0, 1, stream);                                 // d hn += d hp P
    kgpt_gemm(w.dhp, 1, D, w.hn, D, 1, w.dp_part, D, D, D, 2 * B, KGPT_DP_SPLIT, (long)D * D, 0, stream);    // dP = d hp^T hn
    hipLaunchKernelGGL(kgpt_split_sum_kernel, dim3(1024), blk, 0, stream, w.dp_part, dproj, (size_t)D * D, KGPT_DP_SPLIT);
  }
  hipLaunchKernelGGL(kgpt_norm_bwd_kernel, dim3(kgpt_rows_grid(4L * B)), blk, 0, stream, w.drow_ent, w.hn, w.tn, w.norms, B, D);
  const unsigned gy = (unsigned)((D + 1023) / 1024);
  const struct { int kind; const int32_t* order; const float* drow; float* table; int M, n_rows; } seg[2] = {
      {0, ent_order, w.drow_ent, dent, 4 * B, n_ent}, {1, rel_order, w.drow_rel, drel, 2 * B, n_rel}};
  for (const auto& s : seg) {
    const unsigned np = (unsigned)kgpt_pieces(s.M);
    hipLaunchKernelGGL(kgpt_seg_piece_kernel, dim3(np, gy), blk, 0, stream, s.drow, s.order, s.kind, h, nh, t, nt, r, B, s.n_rows, s.table,
                       w.head, w.tail, w.pkeys, s.M, D);
    hipLaunchKernelGGL(kgpt_seg_join_kernel, dim3(np, gy), blk, 0, stream, w.pkeys, s.table, w.head, w.tail, (int)np, D);
  }
  return ia_check_launch();
}

extern "C" int ia_kgpt_adam_l2(float* params, float* grads, float* exp_avg, float* exp_avg_sq, size_t n, float lr, float beta1, float beta2,
                               float eps, float weight_decay, int step, hipStream_t stream) {
  (void)hipGetLastError();
  if (!params || !grads || !exp_avg || !exp_avg_sq || step <= 0) return IA_ERR_ARG;
  if (((uintptr_t)params | (uintptr_t)grads | (uintptr_t)exp_avg | (uintptr_t)exp_avg_sq) & 15) return IA_ERR_ARG;
  if (n == 0) return IA_OK;
  const double bc1 = 1.0 - pow((double)beta1, step), bc2 = 1.0 - pow((double)beta2, step);
  const float step_size = (float)(lr / bc1), bc2_sqrt = (float)sqrt(bc2);
  size_t blocks = (n / 4 + 255) / 256;
  if (blocks < 1) blocks = 1;
  if (blocks > 8192) blocks = 8192;
  hipLaunchKernelGGL(kgpt_adam_l2_kernel, dim3((unsigned)blocks), dim3(256), 0, stream, params, grads, exp_avg, exp_avg_sq, n, beta1, beta2, eps,
                     weight_decay, step_size, bc2_sqrt);
  return ia_check_launch();
}

extern "C" int ia_kgpt_row_normalize(float* x, int rows, int D, hipStream_t stream) {
  (void)hipGetLastError();
  if (!x || rows <= 0 || D <= 0 || (D & 3)) return IA_ERR_ARG;
  hipLaunchKernelGGL(kgpt_row_normalize_kernel, dim3(kgpt_rows_grid(rows)), dim3(256), 0, stream, x, rows, D);
  return ia_check_launch();
}

extern "C" int ia_kgpt_corrupt(const int64_t* h, const int64_t* t, const int64_t* r, int n, const float* bern_probs, int n_probs, int n_ent,
                               uint64_t seed, int64_t* nh, int64_t* nt, hipStream_t stream) {
  (void)hipGetLastError();
  if (!h || !t || !r || !bern_probs || !nh || !nt || n <= 0 || n_probs <= 0 || n_ent < 2) return IA_ERR_ARG;
  hipLaunchKernelGGL(kgpt_corrupt_kernel, dim3((n + 255) / 256), dim3(256), 0, stream, h, t, r, n, bern_probs, n_probs, n_ent, seed, nh, nt);
  return ia_check_launch();
}
