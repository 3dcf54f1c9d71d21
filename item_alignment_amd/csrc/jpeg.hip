// Baseline JPEG decode on the GPU (DESIGN.md §4.7 "JPEG decode"): the entropy-coded scan of a batch of files -> int16 DCT
// coefficients (ia_jpeg_entropy), coefficients -> the uint8 RGB frames Pillow (libjpeg-turbo: accurate integer IDCT, fancy
// upsampling, 16.16 colour conversion) produces, byte for byte (ia_jpeg_reconstruct).  The host (data/jpeg.py) parses the
// headers, removes the stuffed zeros, cuts the scan at its restart markers into 4-byte aligned segments and writes one descriptor
// per image; nothing here trusts the scan itself.
//
// Entropy stage, one workgroup per image.  A restart segment is cut into pieces of `subseq_bits` bits; a piece owns the symbols
// that START inside it.  One step function (state = bit position, block within the MCU, zigzag index) serves every pass:
//   pass A   every piece decodes from its own first bit with state (block 0, k 0); stores its exit state, the blocks it finished
//            and the sum of the DC differences it saw per component
//   pass B   piece i decodes again from the exit state of piece i-1 unless that is the entry it decoded from last time; after
//            round r the first r+1 pieces of every segment are right, so max(pieces of a segment) rounds bound the loop, and a
//            round in which no piece changed ends it early (Huffman streams resynchronise within a few pieces)
//   scan     exclusive per-segment prefix of (blocks, DC sums) over the pieces
//   pass C   every piece decodes a last time and writes its non-zero coefficients, natural order, DC already summed
// Invariants: every loop is bounded by a descriptor field (a step consumes at least one bit, a piece is subseq_bits long); no
// workgroup reads what another one writes; the scan is only ever read through JpegBits, which clamps to the segment and returns
// 1-bits beyond it; coefficient writes go to block numbers below the segment's expected count, which lie inside the image's grids.
#include "common.h"

namespace {

// one Huffman table as the host lays it out (data/jpeg.py huffman_blob): 9-bit look-ahead (length << 8 | symbol, 0 = longer than
// 9 bits), maxcode[l] for l = 0..17 (-1 = no code of that length), valoff[l] = index of the first symbol of length l minus its
// first code, the symbols
constexpr int JT_LUT = 0, JT_MAXCODE = 1024, JT_VALOFF = 1096, JT_VAL = 1164, JT_BYTES = 1424, JT_PER_IMAGE = 6;
constexpr int JD_WORDS = 16;      // descriptor words per image (data/jpeg.py DESC_*)
enum { JD_W, JD_H, JD_NCOMP, JD_HS, JD_VS, JD_MX, JD_MY, JD_RI, JD_NSEG, JD_SEG0, JD_NPIECES, JD_PIECE0, JD_MAXSEGPIECES, JD_COEF, JD_PLANE, JD_OUT };
constexpr int JPEG_GUARD = 64;    // int16 elements left untouched in front of, between and behind the component grids of an image
constexpr int PW_FIELDS = 10;     // per-piece workspace words (structure of arrays, stride = total pieces)
enum { PW_EP, PW_ES, PW_XAP, PW_XAS, PW_XBP, PW_XBS, PW_CNT, PW_DC0, PW_DC1, PW_DC2 };

__constant__ uint8_t kZigzag[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                                    41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                                    30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};

// the only way the scan is read: big-endian dwords of one segment (4-byte aligned start), bytes at or beyond `len` read as 0xFF
struct JpegBits {
  const uint8_t* s;
  int len;
  IA_DEV uint32_t word(int i) const {
    const int b = i * 4;
    if (b + 4 <= len) return __builtin_bswap32(*reinterpret_cast<const uint32_t*>(s + b));
    uint32_t w = 0xFFFFFFFFu;
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (b + j < len) w = (w & ~(0xFFu << (24 - 8 * j))) | ((uint32_t)s[b + j] << (24 - 8 * j));
    return w;
  }
  IA_DEV uint32_t peek(int p) const {      // the 32 bits from bit p on, first bit on top
    const int i = p >> 5, sh = p & 31;
    const uint32_t w0 = word(i);
    return sh ? (w0 << sh) | (word(i + 1) >> (32 - sh)) : w0;
  }
};

struct JpegGeom {      // per image, wave-uniform
  int hs, vs, nl, bpm, mx;      // luma sampling, luma blocks per MCU, blocks per MCU, MCUs per row
  int coff0, coff1, coff2;      // first coefficient of each component's grid (int16 elements)
  IA_DEV int coff(int c) const { return c == 0 ? coff0 : (c == 1 ? coff1 : coff2); }
};

// One symbol.  k == 0: a DC code (category t) and its t bits; else an AC code rs: ZRL adds 16, EOB or k >= 64 ends the block.
// A code that matches nothing reads as 16 bits of symbol 0 (category 0 / end of block) and is an error; so is a coefficient
// whose zigzag index passes 63 (its bits are skipped, the block ends).  Returns bit 0 = block finished, bit 1 = error; `at` =
// zigzag index of the value decoded (-1 none), `comp` = the component the symbol belonged to.
IA_DEV int jpeg_step(const JpegBits& bits, const uint8_t* tabs, const JpegGeom& g, int& p, int& blk, int& k, int& at, int& val, int& comp) {
  comp = blk < g.nl ? 0 : blk - g.nl + 1;
  const uint8_t* T = tabs + (2 * comp + (k != 0)) * JT_BYTES;
  const uint32_t v = bits.peek(p);
  const uint32_t e = reinterpret_cast<const uint16_t*>(T + JT_LUT)[v >> 23];
  int len = 16, sym = 0, flags = 2;
  if (e) {
    len = e >> 8; sym = e & 255; flags = 0;
  } else {
    const int* maxcode = reinterpret_cast<const int*>(T + JT_MAXCODE);
    const int* valoff = reinterpret_cast<const int*>(T + JT_VALOFF);
    for (int l = 10; l <= 16; ++l) {
      const int code = (int)(v >> (32 - l));
      if (code <= maxcode[l]) { sym = T[JT_VAL + ((valoff[l] + code) & 255)]; len = l; flags = 0; break; }
    }
  }
  at = -1; val = 0;
  int s;
  if (k == 0) {
    s = sym & 15; at = 0; k = 1;
  } else {
    s = sym & 15;
    const int r = sym >> 4;
    if (s == 0) {
      k = r == 15 ? k + 16 : 64;
    } else {
      k += r;
      if (k > 63) flags |= 2; else at = k;
      k += 1;
    }
  }
  if (s) {      // len + s <= 31: the extra bits sit in the same 32-bit window
    const int x = (int)((v << len) >> (32 - s));
    val = x >= (1 << (s - 1)) ? x : x - (1 << s) + 1;
  }
  if (at < 0) val = 0;
  p += len + s;
  if (k >= 64) { k = 0; blk = blk + 1 == g.bpm ? 0 : blk + 1; flags |= 1; }
  return flags;
}

// counting decode of one piece (passes A and B): from (p, blk, k) until the position reaches `end`
IA_DEV void jpeg_count_piece(const JpegBits& bits, const uint8_t* tabs, const JpegGeom& g, int end, int& p, int& blk, int& k, int& nblk, int& d0,
                             int& d1, int& d2) {
  nblk = d0 = d1 = d2 = 0;
  while (p < end) {      // <= end - p iterations: a step consumes at least one bit
    int at, val, c;
    const int f = jpeg_step(bits, tabs, g, p, blk, k, at, val, c);
    if (at == 0) { if (c == 0) d0 += val; else if (c == 1) d1 += val; else d2 += val; }
    nblk += f & 1;
  }
}

IA_DEV int16_t* jpeg_block_ptr(int16_t* coef, const JpegGeom& g, int gblock) {
  const int mcu = gblock / g.bpm, b = gblock - mcu * g.bpm;
  const int c = b < g.nl ? 0 : b - g.nl + 1;
  const int hb = c ? 1 : g.hs, vb = c ? 1 : g.vs, bi = c ? 0 : b;
  const int row = (mcu / g.mx) * vb + bi / hb, col = (mcu % g.mx) * hb + bi % hb;
  return coef + g.coff(c) + ((size_t)row * (g.mx * hb) + col) * 64;
}

__global__ __launch_bounds__(256) void jpeg_entropy_kernel(const int* __restrict__ desc, const uint8_t* __restrict__ scan, const int* __restrict__ seg_off,
                                                           const int* __restrict__ seg_len, const int* __restrict__ seg_piece0,
                                                           const int* __restrict__ piece_seg, const uint8_t* __restrict__ tables, int* pw,
                                                           int total_pieces, int16_t* coef, int subseq_bits, int* __restrict__ status,
                                                           int* __restrict__ rounds) {
  __shared__ __attribute__((aligned(16))) uint8_t tabs[JT_PER_IMAGE * JT_BYTES];
  __shared__ uint8_t zz[64];
  __shared__ int part[256][5];      // scan: per thread (has a segment start, blocks, dc0, dc1, dc2)
  __shared__ int sh_status;
  const int img = blockIdx.x, tid = threadIdx.x;
  const int* d = desc + img * JD_WORDS;
  const int ncomp = d[JD_NCOMP], nseg = d[JD_NSEG], seg0 = d[JD_SEG0], np = d[JD_NPIECES], piece0 = d[JD_PIECE0];
  const int ri = d[JD_RI], mcus = d[JD_MX] * d[JD_MY];
  JpegGeom g;
  g.hs = d[JD_HS]; g.vs = d[JD_VS]; g.nl = g.hs * g.vs; g.bpm = ncomp == 1 ? 1 : g.nl + 2; g.mx = d[JD_MX];
  const int nblk_luma = mcus * g.nl, nblk_chroma = mcus;
  g.coff0 = d[JD_COEF];
  g.coff1 = g.coff0 + nblk_luma * 64 + JPEG_GUARD;
  g.coff2 = g.coff1 + nblk_chroma * 64 + JPEG_GUARD;

  {      // tables -> LDS, zigzag -> LDS, the grids -> 0 (the guards between them are left alone)
    const uint32_t* src = reinterpret_cast<const uint32_t*>(tables + (size_t)img * JT_PER_IMAGE * JT_BYTES);
    uint32_t* dst = reinterpret_cast<uint32_t*>(tabs);
    for (int i = tid; i < 2 * ncomp * (JT_BYTES / 4); i += 256) dst[i] = src[i];
    if (tid < 64) zz[tid] = kZigzag[tid];
    if (tid == 0) sh_status = 0;
    for (int c = 0; c < ncomp; ++c) {
      u32x4* z = reinterpret_cast<u32x4*>(coef + g.coff(c));      // grids start at multiples of 8 elements
      const int n16 = (c ? nblk_chroma : nblk_luma) * 8;
      for (int i = tid; i < n16; i += 256) z[i] = u32x4{0, 0, 0, 0};
    }
  }
  __syncthreads();

  int* ws[PW_FIELDS];
#pragma unroll
  for (int f = 0; f < PW_FIELDS; ++f) ws[f] = pw + (size_t)f * total_pieces + piece0;
  const int* pseg = piece_seg + piece0;

  // ---- pass A
  for (int i = tid; i < np; i += 256) {
    JpegBits bits; int j0;
    bits.s = scan + seg_off[seg0 + pseg[i]]; bits.len = seg_len[seg0 + pseg[i]]; j0 = seg_piece0[seg0 + pseg[i]];
    const int nbits = bits.len * 8, j = i - j0;
    int p = j * subseq_bits, blk = 0, k = 0, n, d0, d1, d2;
    const int end = min(p + subseq_bits, nbits);
    ws[PW_EP][i] = p; ws[PW_ES][i] = 0;
    jpeg_count_piece(bits, tabs, g, end, p, blk, k, n, d0, d1, d2);
    ws[PW_XAP][i] = p; ws[PW_XAS][i] = blk | (k << 8);
    ws[PW_CNT][i] = n; ws[PW_DC0][i] = d0; ws[PW_DC1][i] = d1; ws[PW_DC2][i] = d2;
  }
  __syncthreads();

  // ---- pass B: exit states double-buffered (round r reads buffer r & 1, writes the other)
  int nrounds = 0;
  const int max_rounds = d[JD_MAXSEGPIECES];
  for (int r = 0; r < max_rounds; ++r) {
    const bool odd = r & 1;
    int* xp = odd ? ws[PW_XBP] : ws[PW_XAP]; int* xs = odd ? ws[PW_XBS] : ws[PW_XAS];
    int* yp = odd ? ws[PW_XAP] : ws[PW_XBP]; int* ys = odd ? ws[PW_XAS] : ws[PW_XBS];
    int changed = 0;
    for (int i = tid; i < np; i += 256) {
      JpegBits bits; int j0;
      bits.s = scan + seg_off[seg0 + pseg[i]]; bits.len = seg_len[seg0 + pseg[i]]; j0 = seg_piece0[seg0 + pseg[i]];
      const int j = i - j0;
      if (j == 0 || (xp[i - 1] == ws[PW_EP][i] && xs[i - 1] == ws[PW_ES][i])) {      // settled (a segment's first piece always is)
        yp[i] = xp[i]; ys[i] = xs[i];
        continue;
      }
      int p = xp[i - 1], st = xs[i - 1], blk = st & 255, k = st >> 8, n, d0, d1, d2;
      ws[PW_EP][i] = p; ws[PW_ES][i] = st;
      const int end = min((j + 1) * subseq_bits, bits.len * 8);
      jpeg_count_piece(bits, tabs, g, end, p, blk, k, n, d0, d1, d2);
      yp[i] = p; ys[i] = blk | (k << 8);
      ws[PW_CNT][i] = n; ws[PW_DC0][i] = d0; ws[PW_DC1][i] = d1; ws[PW_DC2][i] = d2;
      changed = 1;
    }
    if (!__syncthreads_or(changed)) break;
    ++nrounds;
  }

  // ---- exclusive per-segment scan of (blocks, DC sums) over the pieces: a contiguous run of pieces per thread, the 256 run
  // totals combined by one thread.  The prefixes go where the exit states were (no longer needed).
  const int per = (np + 255) / 256, lo = min(tid * per, np), hi = min(lo + per, np);
  {
    int has = 0, a = 0, b0 = 0, b1 = 0, b2 = 0;
    for (int i = lo; i < hi; ++i) {
      if (i == seg_piece0[seg0 + pseg[i]]) { has = 1; a = b0 = b1 = b2 = 0; }
      a += ws[PW_CNT][i]; b0 += ws[PW_DC0][i]; b1 += ws[PW_DC1][i]; b2 += ws[PW_DC2][i];
    }
    part[tid][0] = has; part[tid][1] = a; part[tid][2] = b0; part[tid][3] = b1; part[tid][4] = b2;
  }
  __syncthreads();
  if (tid == 0) {
    int a = 0, b0 = 0, b1 = 0, b2 = 0;
    for (int t = 0; t < 256; ++t) {      // part[t] <- the carry into run t
      const int has = part[t][0], ta = part[t][1], t0 = part[t][2], t1 = part[t][3], t2 = part[t][4];
      part[t][1] = a; part[t][2] = b0; part[t][3] = b1; part[t][4] = b2;
      if (has) { a = ta; b0 = t0; b1 = t1; b2 = t2; } else { a += ta; b0 += t0; b1 += t1; b2 += t2; }
    }
  }
  __syncthreads();
  {
    int a = part[tid][1], b0 = part[tid][2], b1 = part[tid][3], b2 = part[tid][4];
    for (int i = lo; i < hi; ++i) {
      const int seg = pseg[i];
      if (i == seg_piece0[seg0 + seg]) a = b0 = b1 = b2 = 0;
      const int n = ws[PW_CNT][i], e0 = ws[PW_DC0][i], e1 = ws[PW_DC1][i], e2 = ws[PW_DC2][i];
      ws[PW_XAP][i] = a; ws[PW_XAS][i] = b0; ws[PW_XBP][i] = b1; ws[PW_XBS][i] = b2;
      a += n; b0 += e0; b1 += e1; b2 += e2;
      const bool last = i + 1 == np || pseg[i + 1] != seg;
      if (last && a < min(ri, mcus - seg * ri) * g.bpm) atomicOr(&sh_status, 1);      // the bits ran out before the segment's blocks did
    }
  }
  __syncthreads();

  // ---- pass C
  int err = 0;
  for (int i = tid; i < np; i += 256) {
    JpegBits bits; int j0;
    const int seg = pseg[i];
    bits.s = scan + seg_off[seg0 + seg]; bits.len = seg_len[seg0 + seg]; j0 = seg_piece0[seg0 + seg];
    const int j = i - j0, end = min((j + 1) * subseq_bits, bits.len * 8);
    const int expected = min(ri, mcus - seg * ri) * g.bpm, gbase = seg * ri * g.bpm;
    int p = ws[PW_EP][i], st = ws[PW_ES][i], blk = st & 255, k = st >> 8;
    int nb = ws[PW_XAP][i], d0 = ws[PW_XAS][i], d1 = ws[PW_XBP][i], d2 = ws[PW_XBS][i];
    int16_t* out = nb < expected ? jpeg_block_ptr(coef, g, gbase + nb) : nullptr;
    while (p < end && nb < expected) {      // symbols past the expected blocks (the padding bits) are ignored
      int at, val, c;
      const int f = jpeg_step(bits, tabs, g, p, blk, k, at, val, c);
      err |= f & 2;
      if (at == 0) {
        int dc;
        if (c == 0) dc = (d0 += val); else if (c == 1) dc = (d1 += val); else dc = (d2 += val);
        if (dc) out[0] = (int16_t)dc;
      } else if (at > 0 && val) {
        out[zz[at]] = (int16_t)val;
      }
      if (f & 1) {
        ++nb;
        if (nb < expected) out = jpeg_block_ptr(coef, g, gbase + nb);
      }
    }
  }
  if (err) atomicOr(&sh_status, 2);
  __syncthreads();
  if (tid == 0) { status[img] = sh_status; rounds[img] = nrounds; }
  (void)nseg;
}

// ------------------------------------------------------------------------------------------------------------ reconstruction
constexpr int F0_298 = 2446, F0_390 = 3196, F0_541 = 4433, F0_765 = 6270, F0_899 = 7373, F1_175 = 9633, F1_501 = 12299, F1_847 = 15137,
              F1_961 = 16069, F2_053 = 16819, F2_562 = 20995, F3_072 = 25172;

// libjpeg jidctint.c (accurate integer, CONST_BITS 13, PASS1_BITS 2): one 1-D pass, o = DESCALE(.., N)
template <int N>
IA_DEV void idct_1d(const int* i, int* o) {
  int z1 = (i[2] + i[6]) * F0_541;
  const int t2 = z1 - i[6] * F1_847, t3 = z1 + i[2] * F0_765;
  const int t0 = (i[0] + i[4]) * 8192, t1 = (i[0] - i[4]) * 8192;
  const int t10 = t0 + t3, t13 = t0 - t3, t11 = t1 + t2, t12 = t1 - t2;
  int a0 = i[7], a1 = i[5], a2 = i[3], a3 = i[1];
  z1 = a0 + a3;
  int z2 = a1 + a2, z3 = a0 + a2, z4 = a1 + a3;
  const int z5 = (z3 + z4) * F1_175;
  a0 *= F0_298; a1 *= F2_053; a2 *= F3_072; a3 *= F1_501;
  z1 *= -F0_899; z2 *= -F2_562;
  z3 = z3 * -F1_961 + z5; z4 = z4 * -F0_390 + z5;
  a0 += z1 + z3; a1 += z2 + z4; a2 += z2 + z3; a3 += z1 + z4;
  constexpr int R = 1 << (N - 1);
  o[0] = (t10 + a3 + R) >> N; o[7] = (t10 - a3 + R) >> N;
  o[1] = (t11 + a2 + R) >> N; o[6] = (t11 - a2 + R) >> N;
  o[2] = (t12 + a1 + R) >> N; o[5] = (t12 - a1 + R) >> N;
  o[3] = (t13 + a0 + R) >> N; o[4] = (t13 - a0 + R) >> N;
}

IA_DEV int clamp255(int v) { return v < 0 ? 0 : (v > 255 ? 255 : v); }

// dequantisation + IDCT, one thread per 8 x 8 block: coefficients (natural order) -> the component's uint8 plane over the padded grid.
// grid (blocks of threads per image, images)
__global__ __launch_bounds__(256) void jpeg_idct_kernel(const int* __restrict__ desc, const int16_t* __restrict__ coef, const uint8_t* __restrict__ qt,
                                                        uint8_t* __restrict__ planes) {
  __shared__ int q[3][64];
  const int img = blockIdx.y;
  const int* d = desc + img * JD_WORDS;
  const int ncomp = d[JD_NCOMP], nl = d[JD_HS] * d[JD_VS], mx = d[JD_MX], mcus = mx * d[JD_MY];
  if ((int)threadIdx.x < ncomp * 64) q[threadIdx.x >> 6][threadIdx.x & 63] = qt[(size_t)img * 192 + threadIdx.x];
  __syncthreads();
  const int nluma = mcus * nl, total = ncomp == 1 ? nluma : nluma + 2 * mcus;
  for (int t = blockIdx.x * 256 + threadIdx.x; t < total; t += gridDim.x * 256) {
    const int c = t < nluma ? 0 : (t - nluma < mcus ? 1 : 2);
    const int b = c == 0 ? t : t - nluma - (c - 1) * mcus;
    const int bw = c ? mx : mx * d[JD_HS];
    const int16_t* src = coef + d[JD_COEF] + (c ? nluma * 64 + JPEG_GUARD + (c - 1) * (mcus * 64 + JPEG_GUARD) : 0) + (size_t)b * 64;
    uint8_t* dst = planes + d[JD_PLANE] + (size_t)(c ? nluma + (c - 1) * mcus : 0) * 64 + ((size_t)(b / bw) * 8 * bw + (b % bw)) * 8;
    int x[64];
#pragma unroll
    for (int r = 0; r < 8; ++r) {
      const s16x8 v = *reinterpret_cast<const s16x8*>(src + r * 8);
#pragma unroll
      for (int e = 0; e < 8; ++e) x[r * 8 + e] = (int)v[e] * q[c][r * 8 + e];
    }
#pragma unroll
    for (int col = 0; col < 8; ++col) {      // pass 1 down the columns
      int in[8], o[8];
#pragma unroll
      for (int r = 0; r < 8; ++r) in[r] = x[r * 8 + col];
      idct_1d<11>(in, o);
#pragma unroll
      for (int r = 0; r < 8; ++r) x[r * 8 + col] = o[r];
    }
#pragma unroll
    for (int r = 0; r < 8; ++r) {            // pass 2 along the rows, + 128, clamp
      int o[8];
      idct_1d<18>(x + r * 8, o);
      uint32_t lo = 0, hi = 0;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        lo |= (uint32_t)clamp255(o[e] + 128) << (8 * e);
        hi |= (uint32_t)clamp255(o[e + 4] + 128) << (8 * e);
      }
      *reinterpret_cast<u32x2*>(dst + (size_t)r * bw * 8) = u32x2{lo, hi};
    }
  }
}

// libjpeg jdsample.c h2v1_fancy_upsample / h2v2_fancy_upsample at output position (x, y) of a chroma plane cw x ch (pitch bytes a
// row); planes at most 2 samples wide are replicated instead
IA_DEV int chroma_h2v1(const uint8_t* P, int pitch, int cw, int x, int y) {
  const uint8_t* row = P + (size_t)y * pitch;
  const int i = x >> 1;
  if (cw <= 2) return row[i];
  if (x & 1) return i == cw - 1 ? row[i] : (3 * row[i] + row[i + 1] + 2) >> 2;
  return i == 0 ? row[0] : (3 * row[i] + row[i - 1] + 1) >> 2;
}
IA_DEV int chroma_h2v2(const uint8_t* P, int pitch, int cw, int ch, int x, int y) {
  const int i = x >> 1, j = y >> 1;
  if (cw <= 2) return P[(size_t)j * pitch + i];
  const int jo = (y & 1) ? min(j + 1, ch - 1) : max(j - 1, 0);
  const uint8_t* r0 = P + (size_t)j * pitch;
  const uint8_t* r1 = P + (size_t)jo * pitch;
  const int s = 3 * r0[i] + r1[i];
  if (x & 1) return i == cw - 1 ? (4 * s + 7) >> 4 : (3 * s + 3 * r0[i + 1] + r1[i + 1] + 7) >> 4;
  return i == 0 ? (4 * s + 8) >> 4 : (3 * s + 3 * r0[i - 1] + r1[i - 1] + 8) >> 4;
}

// upsampling + YCbCr -> RGB (jdcolor.c, 16.16 fixed point), one thread per pixel; gray is written three times
__global__ __launch_bounds__(256) void jpeg_color_kernel(const int* __restrict__ desc, const uint8_t* __restrict__ planes, uint8_t* __restrict__ out) {
  const int* d = desc + blockIdx.y * JD_WORDS;
  const int W = d[JD_W], H = d[JD_H], ncomp = d[JD_NCOMP], hs = d[JD_HS], vs = d[JD_VS], mx = d[JD_MX], mcus = mx * d[JD_MY];
  const uint8_t* Y = planes + d[JD_PLANE];
  const int ypitch = mx * hs * 8, cpitch = mx * 8;
  const uint8_t* Cb = Y + (size_t)mcus * hs * vs * 64;
  const uint8_t* Cr = Cb + (size_t)mcus * 64;
  const int cw = (W + hs - 1) / hs, ch = (H + vs - 1) / vs;
  uint8_t* o = out + d[JD_OUT];
  const int npix = W * H;
  for (int t = blockIdx.x * 256 + threadIdx.x; t < npix; t += gridDim.x * 256) {
    const int y = t / W, x = t - y * W;
    const int yy = Y[(size_t)y * ypitch + x];
    int r = yy, g = yy, b = yy;
    if (ncomp == 3) {
      int cb, cr;
      if (hs == 1) { cb = Cb[(size_t)y * cpitch + x]; cr = Cr[(size_t)y * cpitch + x]; }
      else if (vs == 1) { cb = chroma_h2v1(Cb, cpitch, cw, x, y); cr = chroma_h2v1(Cr, cpitch, cw, x, y); }
      else { cb = chroma_h2v2(Cb, cpitch, cw, ch, x, y); cr = chroma_h2v2(Cr, cpitch, cw, ch, x, y); }
      cb -= 128; cr -= 128;
      r = clamp255(yy + ((91881 * cr + 32768) >> 16));
      b = clamp255(yy + ((116130 * cb + 32768) >> 16));
      g = clamp255(yy + ((-22554 * cb + 32768 - 46802 * cr) >> 16));
    }
    uint8_t* px = o + (size_t)t * 3;
    px[0] = (uint8_t)r; px[1] = (uint8_t)g; px[2] = (uint8_t)b;
  }
}

}  // namespace

// Entropy stage of a batch of baseline JPEG scans (layouts: item_alignment_amd/data/jpeg.py).  desc [n_images][16] int32; scan =
// the unstuffed restart segments of all images, each starting at a multiple of 4 bytes; seg_off / seg_len / seg_piece0 per segment
// (byte offset into scan, byte length, image-local index of its first piece); piece_seg per piece (image-local segment); tables
// [n_images][6][1424] bytes; piece_ws: 10 * total_pieces int32 of scratch; coef: int16, the component grids of every image at
// desc[JD_COEF] with 64 untouched elements in front of, between and behind them.  status [n_images]: 0 = every block decoded;
// rounds [n_images]: pass-B rounds that still changed a piece.
extern "C" int ia_jpeg_entropy(const int* desc, int n_images, const uint8_t* scan, const int* seg_off, const int* seg_len, const int* seg_piece0,
                               const int* piece_seg, const uint8_t* tables, int* piece_ws, int total_pieces, int16_t* coef, int subseq_bits,
                               int* status, int* rounds, hipStream_t stream) {
  (void)hipGetLastError();
  if (!desc || !scan || !seg_off || !seg_len || !seg_piece0 || !piece_seg || !tables || !piece_ws || !coef || !status || !rounds) return IA_ERR_ARG;
  if (n_images <= 0 || total_pieces <= 0 || subseq_bits < 64 || subseq_bits % 32 != 0) return IA_ERR_ARG;
  hipLaunchKernelGGL(jpeg_entropy_kernel, dim3(n_images), dim3(256), 0, stream, desc, scan, seg_off, seg_len, seg_piece0, piece_seg, tables, piece_ws,
                     total_pieces, coef, subseq_bits, status, rounds);
  return ia_check_launch();
}

// Coefficients -> RGB: dequantisation (qt [n_images][3][64], natural order) + IDCT into `planes` (scratch: one byte per coefficient,
// each image's at desc[JD_PLANE]), then upsampling + colour conversion into out at desc[JD_OUT] ([H, W, 3] per image).
extern "C" int ia_jpeg_reconstruct(const int* desc, int n_images, const int16_t* coef, const uint8_t* qt, uint8_t* planes, uint8_t* out,
                                   hipStream_t stream) {
  (void)hipGetLastError();
  if (!desc || !coef || !qt || !planes || !out || n_images <= 0 || n_images > 65535) return IA_ERR_ARG;
  hipLaunchKernelGGL(jpeg_idct_kernel, dim3(8, n_images), dim3(256), 0, stream, desc, coef, qt, planes);
  hipLaunchKernelGGL(jpeg_color_kernel, dim3(32, n_images), dim3(256), 0, stream, desc, planes, out);
  return ia_check_launch();
}
